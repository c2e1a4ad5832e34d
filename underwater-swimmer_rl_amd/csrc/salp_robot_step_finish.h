// salp_robot_step_finish.h — the end of an env step behind its cycle (salp_robot_step_body.h; the rollout kernel of
// salp_robot_kernels.h includes it at its service points): reward, termination and truncation, the terminal row of
// final_obs and the same-step autoreset.  Reads r, P, i, genv, active, final_obs (the rows of this step); leaves rew, term,
// trunc and the float row o[6].  No include guard: included text.
  // _calculate_reward (:203-243) and termination (:171-185)
  const double dx = r.pos[0] - r.target[0], dy = r.pos[1] - r.target[1];
  const double dist = sqrt(dx * dx + dy * dy);
  const double r_track = (-dist + r.prev_dist) * 100;
  r.prev_dist = dist;
  const double ex = -(dx / (dist + 1e-6)), ey = -(dy / (dist + 1e-6));
  const double vn = sqrt(r.vw[0] * r.vw[0] + r.vw[1] * r.vw[1]);
  const double r_heading = (r.vw[0] / (vn + 1e-6)) * ex + (r.vw[1] / (vn + 1e-6)) * ey;
  double rew = r_track + 0.5 * r_heading;
  bool term = false, trunc = false;
  if (dist < 0.01) { term = true; rew += 10.0; }
  else if (dist > 5.0) { trunc = true; rew -= 5.0; }
  if (r.cycle >= P.max_cycles) trunc = true;

  float o[6];
  if (term || trunc) {
    if (final_obs && active) {
      observe_robot(r, o);
#pragma unroll
      for (int k = 0; k < 6; ++k) final_obs[i * 6 + k] = o[k];
    }
    reset_robot(r, P, genv);
  }
