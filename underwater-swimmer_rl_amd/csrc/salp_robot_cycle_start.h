// salp_robot_cycle_start.h — third piece of one breathing cycle (salp_robot_cycle_body.h): the phase boundaries, the
// shape-dependent quantities the Euler step carries, the exact sin / cos of the Euler angles at the cycle start and
// sample 0 of a recorded history.  Reads what the two pieces before it left, and kRecord, H, i.  No include guard:
// included text.
  const double t_jet_end = refill_time + jet_time, t_coast_end = t_jet_end + coast_time;
  double mass = 0, inv_m = 0, kd = 0, ktc = 0, ax = 0, I0 = 0, I1 = 0, I2 = 0, iI0 = 0, iI1 = 0, iI2 = 0;
  bool settled = false;    // the previous step of this lane already had the rest shape (and prevI == I)
  // sin / cos of the three Euler angles are carried through the cycle: exact at its start, then advanced by each
  // step's increment with advance_euler_sincos (salp_fp64_math.h; increments are ~1e-3 rad; an increment above
  // kRotateMaxStep = 0.125 rad anywhere in the wavefront takes the exact path for that step).  Over a whole cycle the
  // carried pair stays within 1e-12 of sin / cos of the exact angle (start + sum of increments).  Against sin / cos
  // of r.eul itself, which the reference takes, the rounding of `eul += d` comes on top: up to steps * ulp(|eul|) / 2,
  // 1.3e-9 per cycle for a yaw wound up to 1e4 rad (measured 3.8e-11) — far inside parity (tests/test_robot_math.py).
  double sp, cp, st, ct, ss, cs;
  sincos_euler(r.eul[0], sp, cp);
  sincos_euler(r.eul[1], st, ct);
  sincos_euler(r.eul[2], ss, cs);
  // history: sample 0 is the state after set_control, with the rest shape and REST (include/salp_robot.h); then
  // one sample every `stride` Euler steps and one after the last step.  Only lanes of the recorded range store;
  // a wavefront without such a lane skips the block on a wave-uniform test.
  const bool rec = kRecord && active && (uint64_t)(i - H.begin) < (uint64_t)H.count;
  const int64_t hj = i - H.begin;   // row of this env in the history
  int32_t n_samples = 0, until_sample = 0;
  const float yaw_f = (float)yaw;
  if constexpr (kRecord) {
    if (__any(rec)) {
      if (rec) {
        store_history_sample(H, hj, 0, r, P.init_length, P.init_width, 3, yaw_f);
        n_samples = 1;
        until_sample = H.stride;
      }
    }
  }
