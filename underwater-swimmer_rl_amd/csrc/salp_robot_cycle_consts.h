// salp_robot_cycle_consts.h — second piece of one breathing cycle (salp_robot_cycle_body.h): what the Euler step needs of
// the physical parameters alone (P), the same in every cycle of a robot.  The rollout kernel of salp_robot_kernels.h
// includes it once in front of its loop.  No include guard: included text.
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
