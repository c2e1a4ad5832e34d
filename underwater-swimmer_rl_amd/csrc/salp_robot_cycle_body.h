// salp_robot_cycle_body.h — one breathing cycle of one robot, included inside the three kernels of salp_robot_kernels.h
// that run one: nozzle.solve_angles + Robot.set_control + Robot.step_through_cycle (robot.py:55-85, 335-358, 422-445).
//   salp_robot_step_kernel, salp_robot_step_record_kernel   through salp_robot_step_body.h (env step)
//   salp_robot_trajectory_kernel                            once per cycle of the trajectory (compare_trajectories.py)
// It reads the enclosing kernel's names: Rb r (the robot, advanced in place), P (physical parameters: the kernel
// argument in the step kernels, this lane's own copy in the trajectory kernel), the cycle's action in physical units
// `contraction` (m), `coast_time` (s), `yaw` (rad), `active` (false on padding lanes, which run no Euler step), and
// for the history kRecord, H and i.  It leaves `steps` (Euler steps of the cycle) and the locals of the cycle in scope.
// Included text rather than a function for the reason given at the top of salp_robot_step_body.h.
// No include guard: included once per kernel (per cycle loop).
  // Nozzle.solve_angles (robot.py:55-85): target = R_br^T @ -(cos yaw, sin yaw, 0) = (-0, -sin yaw, cos yaw).
  // Every angle here is within [-pi, pi]: sincos_small (salp_fp64_math.h) is within 2^-52 absolute of sin / cos there.
  {
    double sy, cy;
    sincos_small(yaw, sy, cy);
    const double t1 = -sy, t2 = cy;
    double a2 = acos(clipd(2 * t2 - 1, -1.0, 1.0));
    if (a2 <= -kPi) a2 += 2 * kPi; else if (a2 > kPi) a2 -= 2 * kPi;
    double a1 = 0.0;
    if (a2 != 0.0) {
      double sa2, ca2;
      sincos_small(a2, sa2, ca2);
      const double a = 0.5 * (ca2 - 1);
      const double b = sqrt(2.0) * sa2 / 2;
      a1 = asin(clipd(t1 / sqrt(a * a + b * b), -1.0, 1.0)) - atan2(b, a);
    }
    if (a1 <= -kPi) a1 += 2 * kPi; else if (a1 > kPi) a1 -= 2 * kPi;
    r.angle1 = a1; r.angle2 = a2;
  }
  // Nozzle.get_nozzle_direction (robot.py:115-130): R_br @ R_mb @ R_nm @ (cos g, 0, sin g), constant over the cycle
  double dir[3];
  {
    double cg, sg, c2, s2, c1, s1;
    sincos_small(P.nz_gamma, sg, cg);
    sincos_small(r.angle2, s2, c2);
    sincos_small(r.angle1, s1, c1);
    // R_nm = R_theta_fixed @ R_nozzle(angle2); v1 = R_nm @ (cg, 0, sg)
    const double nx = (cg * c2) * cg + (-sg) * sg;
    const double ny = s2 * cg;
    const double nzv = (sg * c2) * cg + cg * sg;
    // R_mb = rotation about z by angle1
    const double mx = c1 * nx + (-s1) * ny, my = s1 * nx + c1 * ny, mz = nzv;
    // R_br = [[0,0,-1],[0,1,0],[1,0,0]]
    dir[0] = -mz; dir[1] = my; dir[2] = mx;
  }
  // Robot.set_control (robot.py:335-358)
  r.cycle += 1;
  const double contract_rate = kContractRate, release_rate = kReleaseRate;   // salp_robot_params.h
  const double refill_time = contraction / contract_rate;
  const double jet_time = contraction / release_rate;
  // The cycle length comes straight from the caller's action.  Inside the action Box [0, 1]^3 it is at most
  // 0.06 * 75 + 10 = 14.5 s; the device loop below is bounded by that maximum (kMaxCycleTime), so an unsquashed
  // or diverged policy output (1e9, +inf) cannot spin a wavefront for ever — the reference would stall ONE CPU
  // env for the corresponding 1e11 Euler steps; here a cycle longer than the Box allows is cut at the Box
  // maximum (include/salp_robot.h).  A non-finite length runs no Euler step at all.
  double total = active ? refill_time + jet_time + coast_time : 0.0;   // padding lanes do not step
  total = (total <= kMaxCycleTime) ? total : ((total > kMaxCycleTime) ? kMaxCycleTime : 0.0);
  double cycle_time = 0.0;
  int steps = 0;
  const double dt = P.dt;

  // Robot.step_through_cycle (robot.py:422-445): lanes finish at different times.
  //  * quantities that depend only on the body shape (mass, inertia, drag factors and their reciprocals)
  //    are kept in registers and recomputed only on a step where some lane's shape moves or has just
  //    stopped moving; during coast / rest (most of a cycle) the whole wavefront skips that block;
  //  * sin/cos of the Euler angles are carried from step to step (see advance_euler_sincos below in the loop);
  //  * divisions by dt, by cos(pitch) and by the mass / inertia diagonal are reciprocals (Newton-refined
  //    v_rcp_f64) times a product: a few ulp from the reference's quotient, far inside the parity
  //    tolerance, which is a tolerance already because the reference multiplies 3x3 blocks through BLAS.
  const double inv_dt = rcp_nr(dt);
  const double init_aspect = P.init_length / P.init_width;
  const double contracted_length = P.init_length - P.max_contraction;
  const double min_aspect = contracted_length / (P.init_length - contracted_length + P.init_width);
  const double inv_aspect_span = rcp_nr(init_aspect - min_aspect);
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
#pragma unroll 1
  while (__any(cycle_time < total)) {
    if (cycle_time < total) {
      // Robot.step (robot.py:387-396)
      cycle_time += dt;
      r.time += dt;
      int state;   // update_state :360-373
      if (cycle_time <= refill_time) state = 0;
      else if (cycle_time <= t_jet_end) state = 1;
      else if (cycle_time <= t_coast_end) state = 2;
      else state = 3;
      double jf0 = 0.0, jf1 = 0.0, jf2 = 0.0, td0 = 0.0, td1 = 0.0, td2 = 0.0;
      if (__any(state < 2 || !settled)) {
        // update_properties :375-385
        const double prev_volume = r.volume;
        double length, width;
        if (state == 0) { length = P.init_length - cycle_time * contract_rate; width = P.init_width + cycle_time * contract_rate; }
        else if (state == 1) {
          length = P.init_length - contraction + (cycle_time - refill_time) * release_rate;
          width = P.init_width + contraction - (cycle_time - refill_time) * release_rate;
        } else { length = P.init_length; width = P.init_width; }
        const double hl = length / 2, hw = width / 2;
        const double area = kPi * hl * hw;
        r.volume = water_volume(length, width);
        const double water_mass = P.density * r.volume;
        mass = P.dry_mass + water_mass + P.nz_mass;
        inv_m = rcp_nr(mass);
        // drag coefficient, robot.py:627-649
        const double aspect = length * rcp_nr(width);
        const double nr = clipd((aspect - min_aspect) * inv_aspect_span, 0.0, 1.0);
        const double cd = P.cd_max - nr * (P.cd_max - P.cd_min);
        kd = -0.5 * P.density * area * cd;
        ktc = -P.density * cd * hw * sq(sq(hl));
        if (state == 1) {   // jet force, :494-505
          const double volume_rate = -(r.volume - prev_volume) * inv_dt;
          const double jet_speed = volume_rate / P.nz_area;
          const double mass_rate = (water_mass - prev_volume * P.density) * inv_dt;
          jf0 = 0.1 * mass_rate * (dir[0] * jet_speed);
          jf1 = 0.1 * mass_rate * (dir[1] * jet_speed);
          jf2 = 0.1 * mass_rate * (dir[2] * jet_speed);
        }
        ax = arm_x(P, length);
        double I[3];
        inertia_diag(P, mass, length, width, ax * ax, I);
        I0 = I[0]; I1 = I[1]; I2 = I[2];
        iI0 = rcp_nr(I0); iI1 = rcp_nr(I1); iI2 = rcp_nr(I2);
        td0 = ((I0 - r.prevI[0]) * inv_dt) * r.om[0];
        td1 = ((I1 - r.prevI[1]) * inv_dt) * r.om[1];
        td2 = ((I2 - r.prevI[2]) * inv_dt) * r.om[2];
        r.prevI[0] = I0; r.prevI[1] = I1; r.prevI[2] = I2;
        settled = state >= 2;
      }
      // _newton_equations :494-505
      const double wxv0 = r.om[1] * r.vel[2] - r.om[2] * r.vel[1];
      const double wxv1 = r.om[2] * r.vel[0] - r.om[0] * r.vel[2];
      const double wxv2 = r.om[0] * r.vel[1] - r.om[1] * r.vel[0];
      const double vnorm = sqrt_nr(r.vel[0] * r.vel[0] + r.vel[1] * r.vel[1] + r.vel[2] * r.vel[2]);
      const double kq = kd * vnorm;
      const double acc0 = inv_m * (jf0 + (kq * r.vel[0] + kd * r.vel[0]) + mass * wxv0);
      const double acc1 = inv_m * (jf1 + (kq * r.vel[1] + kd * r.vel[1]) + mass * wxv1);
      const double acc2 = inv_m * (jf2 + (kq * r.vel[2] + kd * r.vel[2]) + mass * wxv2);
      // _euler_equations :507-522
      const double Iw0 = I0 * r.om[0], Iw1 = I1 * r.om[1], Iw2 = I2 * r.om[2];
      const double c0 = r.om[1] * Iw2 - r.om[2] * Iw1;
      const double c1 = r.om[2] * Iw0 - r.om[0] * Iw2;
      const double c2 = r.om[0] * Iw1 - r.om[1] * Iw0;
      const double wnorm = sqrt_nr(r.om[0] * r.om[0] + r.om[1] * r.om[1] + r.om[2] * r.om[2]);
      const double kt = ktc * wnorm;
      // jet torque = arm x jet_force, arm = (ax, 0, 0)
      const double jt1 = -ax * jf2, jt2 = ax * jf1;
      const double al0 = iI0 * (kt * r.om[0] + -c0 - td0);
      const double al1 = iI1 * (jt1 + kt * r.om[1] + -c1 - td1);
      const double al2 = iI2 * (jt2 + kt * r.om[2] + -c2 + 0.1 * vnorm - td2);
      // _update_motion_states :524-532
      r.vel[0] += acc0 * dt; r.vel[1] += acc1 * dt; r.vel[2] += acc2 * dt;
      r.om[0] += al0 * dt; r.om[1] += al1 * dt; r.om[2] += al2 * dt;
      {
        const double ict = rcp_nr(ct);
        const double tt = st * ict;
        const double e0 = r.om[0] + (sp * tt) * r.om[1] + (cp * tt) * r.om[2];
        const double e1 = cp * r.om[1] + (-sp) * r.om[2];
        const double e2 = (sp * ict) * r.om[1] + (cp * ict) * r.om[2];
        const double d0 = e0 * dt, d1 = e1 * dt, d2 = e2 * dt;
        r.eul[0] += d0; r.eul[1] += d1; r.eul[2] += d2;
        advance_euler_sincos(r.eul[0], r.eul[1], r.eul[2], d0, d1, d2, sp, cp, st, ct, ss, cs);
      }
      {
        // R = R_z @ R_y @ R_x
        const double r00 = cs * ct, r01 = cs * st * sp - ss * cp, r02 = cs * st * cp + ss * sp;
        const double r10 = ss * ct, r11 = ss * st * sp + cs * cp, r12 = ss * st * cp - cs * sp;
        const double r20 = -st, r21 = ct * sp, r22 = ct * cp;
        r.vw[0] = r00 * r.vel[0] + r01 * r.vel[1] + r02 * r.vel[2];
        r.vw[1] = r10 * r.vel[0] + r11 * r.vel[1] + r12 * r.vel[2];
        r.vw[2] = r20 * r.vel[0] + r21 * r.vel[1] + r22 * r.vel[2];
      }
      r.pos[0] += r.vw[0] * dt; r.pos[1] += r.vw[1] * dt; r.pos[2] += r.vw[2] * dt;
      ++steps;
      if constexpr (kRecord) {
        const bool take = rec && (--until_sample == 0 || !(cycle_time < total));
        if (__any(take)) {
          if (take) {
            // the shape of update_properties (robot.py:702-735), recomputed with the same operations
            double length = P.init_length, width = P.init_width;
            if (state == 0) { length = P.init_length - cycle_time * contract_rate; width = P.init_width + cycle_time * contract_rate; }
            else if (state == 1) {
              length = P.init_length - contraction + (cycle_time - refill_time) * release_rate;
              width = P.init_width + contraction - (cycle_time - refill_time) * release_rate;
            }
            store_history_sample(H, hj, n_samples, r, length, width, state, yaw_f);
            ++n_samples;
            until_sample = H.stride;
          }
        }
      }
    }
  }
