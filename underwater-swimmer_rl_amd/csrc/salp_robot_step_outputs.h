// salp_robot_step_outputs.h — the stores of an env step of an active lane, behind salp_robot_step_finish.h: the observation
// row (the next episode's first one after an autoreset), reward, flags and the Euler-step count.  obs, reward, terminated,
// truncated and inner_steps are the rows of this step, each nullable.  No include guard: included text.
    observe_robot(r, o);
    if (obs) {
#pragma unroll
      for (int k = 0; k < 6; ++k) obs[i * 6 + k] = o[k];
    }
    if (reward) reward[i] = (float)rew;
    if (terminated) terminated[i] = term ? 1 : 0;
    if (truncated) truncated[i] = trunc ? 1 : 0;
    if (inner_steps) inner_steps[i] = steps;
