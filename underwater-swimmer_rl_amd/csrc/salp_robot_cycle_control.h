// salp_robot_cycle_control.h — first piece of one breathing cycle (salp_robot_cycle_body.h; the rollout kernel of
// salp_robot_kernels.h includes the pieces one by one): nozzle.solve_angles, the jet direction and Robot.set_control with
// the cycle-length guard.  Reads r, P, `contraction`, `coast_time`, `yaw`, `active`; leaves dir, refill_time, jet_time,
// total, cycle_time and steps.  No include guard: included text.
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
