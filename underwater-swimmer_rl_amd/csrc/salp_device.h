// salp_device.h — device-side arithmetic of one SALP swimmer (one env per lane), gfx950.
//
// Restates, for the GPU, the per-step arithmetic of the reference's
//   scripts/utilities/salp_robot.py  ("legacy", SalpRobotEnv.step and helpers, :119-352)
//   src/salp/environments/salp_snake_env.py ("snake", SalpSnakeEnv.step and helpers, :157-428)
//
// Numerics contract:
//   * everything that feeds back into the state (nozzle, breathing, thrust, drag/integration,
//     wall bounce, food placement) is IEEE fp64 in the reference's operation order; these files are
//     compiled with -ffp-contract=off so no multiply-add is fused unless written as fma().
//     The only departures from the reference's fp64 bit pattern are the device sin/cos (<=2 ulp
//     vs glibc) and squared-distance predicates (d^2 < t^2 instead of sqrt(d^2) < t).
//   * quantities that only leave the simulator (observation, reward shaping term) are derived
//     from that fp64 state and finished in fp32.
//
// This file is the umbrella: every unit of the snake simulator includes it and sees the headers below, in this order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "salp_fp64_math.h"   // sincos_small

#include "salp_exp.h"          // the experiment builds' macros: SALP_STAMP*, SALP_COUNT
#include "salp_params.h"       // breathing word, DevParams / StdConsts / CV(), state layout, statistics slots; config -> DevParams
#include "salp_philox.h"       // Philox4x32-10, u53
#include "salp_snake_math.h"   // pymax / pymin, thrust table, sincos_small_t, sin_nozzle_t, atan2_fast, cos_wrapped
#include "salp_env.h"          // wave_sync, EnvCore / Env, load / store, draw stream, shape_of, place_food, reset
#include "salp_step.h"         // jet thrust, step_head / step_tail / step_env, observe
