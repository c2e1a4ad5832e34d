// salp_robot_euler_step.h — one explicit-Euler step of one robot (Robot.step, robot.py:387-396), the body of the loop of
// salp_robot_cycle_body.h and of the rollout kernel's loop (salp_robot_kernels.h), run by the lanes with
// cycle_time < total.  Reads and advances what the three cycle pieces left in scope.  No include guard: included text.
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
