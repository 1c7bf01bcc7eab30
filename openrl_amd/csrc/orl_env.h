// orl_env.h - the device-resident single-agent envs (synthetic fixed-step env of SURVEY.md section 8d, CartPole-v1,
// Pendulum-v1, Acrobot-v1, MountainCar-v0, MountainCarContinuous-v0) as per-env device functions, shared by the fused rollout kernels (orl_act.hip: default towers,
// orl_gen_fused.hip: general towers) and the stand-alone env kernels: one definition, so every route steps an env with the same arithmetic and the
// same Philox streams.  Not part of the C ABI.
#pragma once
#include "orl_common.h"
#include "orl_mlp.h"

namespace orl {

// --------------------------------------------------------------------------------------------------
// Device-resident envs.  State lives in `env_state[N][W]`; one lane (q == 0) owns one env.
// --------------------------------------------------------------------------------------------------
constexpr int SYNTH_STATE_W = 4;     // {steps_in_episode, -, -, -}
constexpr int CARTPOLE_STATE_W = 8;  // {x, x_dot, theta, theta_dot, steps_in_episode, episodes, -, -}
constexpr int PENDULUM_STATE_W = 4;  // {th, thdot, steps_in_episode, episodes}

// synthetic obs component block b (4 normals) for (env, global time t)
__device__ inline void synth_obs_block(uint64_t seed, uint32_t env, uint64_t t, uint32_t b, float (&o)[4]) {
  const u4 r = philox4x32_10(seed, env, 0x0B5E0000u + b, (uint32_t)t, (uint32_t)(t >> 32));
  box_muller(r.x, r.y, o[0], o[1]);
  box_muller(r.z, r.w, o[2], o[3]);
}
__device__ inline float synth_reward(uint64_t seed, uint32_t env, uint64_t t) {
  const u4 r = philox4x32_10(seed, env, 0x4E3A0000u, (uint32_t)t, (uint32_t)(t >> 32));
  return u01(r.x);
}

// CartPole-v1 (gymnasium/envs/classic_control/cartpole.py, euler integrator) in fp32.
__device__ inline void cartpole_reset(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[4]) {
  const u4 r = philox4x32_10(seed, env, 0xCA470000u, episode, 0u);
  s[0] = u01(r.x) * 0.1f - 0.05f;
  s[1] = u01(r.y) * 0.1f - 0.05f;
  s[2] = u01(r.z) * 0.1f - 0.05f;
  s[3] = u01(r.w) * 0.1f - 0.05f;
}
// The step in two halves (round 6): everything that does not depend on the ACTION - the trigonometry of the pole angle and
// the terms built on it - and the rest.  The fused rollout computes the first half on a service wave while the policy is
// still working on the step's action (orl_rollout2.h); cartpole_step() is the composition, so every route steps an env
// through the same expressions.
struct CartPolePre {
  float costh, sinth, t1, den;  // cos / sin of theta, polemass_length * theta_dot^2 * sin, the angular denominator
};
__device__ inline CartPolePre cartpole_pre(const float (&s)[4]) {
  const float masspole = 0.1f, total_mass = 1.1f, length = 0.5f, polemass_length = 0.05f;
  CartPolePre p;
  p.costh = cosf(s[2]);
  p.sinth = sinf(s[2]);
  p.t1 = polemass_length * s[3] * s[3] * p.sinth;
  p.den = length * (4.0f / 3.0f - masspole * p.costh * p.costh / total_mass);
  return p;
}
__device__ inline bool cartpole_post(float (&s)[4], const CartPolePre& p, int action) {
  const float gravity = 9.8f, total_mass = 1.1f, polemass_length = 0.05f, force_mag = 10.0f, tau = 0.02f;
  const float force = action == 1 ? force_mag : -force_mag;
  const float temp = (force + p.t1) / total_mass;
  const float thetaacc = (gravity * p.sinth - p.costh * temp) / p.den;
  const float xacc = temp - polemass_length * thetaacc * p.costh / total_mass;
  s[0] = s[0] + tau * s[1];
  s[1] = s[1] + tau * xacc;
  s[2] = s[2] + tau * s[3];
  s[3] = s[3] + tau * thetaacc;
  const float th_lim = 12.0f * 2.0f * 3.14159265358979323846f / 360.0f;
  return (s[0] < -2.4f) || (s[0] > 2.4f) || (s[2] < -th_lim) || (s[2] > th_lim);
}
__device__ inline bool cartpole_step(float (&s)[4], int action) {
  const CartPolePre p = cartpole_pre(s);
  return cartpole_post(s, p, action);
}


// Pendulum-v1 (gymnasium/envs/classic_control/pendulum.py: max_speed 8, max_torque 2, dt 0.05, g 10, m 1, l 1) in fp32.
// Reset: th ~ U(-pi, pi), thdot ~ U(-1, 1) from the engine's own Philox stream keyed (seed, env, episode) - not gymnasium's
// np_random, as for CartPole.
//
// Deviation (fp32): gymnasium keeps th unwrapped in float64.  Here th is wrapped back to [-pi, pi) after every step
// (pendulum_wrap: one conditional +-2 pi; |th + dt thdot| <= pi + 0.4 never needs more).  In real arithmetic nothing changes
// - cos, sin and angle_normalize are 2 pi-periodic - but an unwrapped fp32 th after a few turns (|th| up to ~80 rad in an
// episode) loses ~6 bits of the dt * thdot increment and pushes sinf / cosf (-ffast-math) into their weak range reduction.
constexpr float PEND_PI = 3.14159265358979323846f, PEND_2PI = 6.28318530717958647692f;
__device__ inline void pendulum_reset(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[2]) {
  const u4 r = philox4x32_10(seed, env, 0x9E4D0000u, episode, 0u);
  s[0] = fmaf(u01(r.x), PEND_2PI, -PEND_PI);
  s[1] = fmaf(u01(r.y), 2.0f, -1.0f);
}
// angle_normalize(x) = ((x + pi) mod 2 pi) - pi with Python's FLOORED modulo: fmodf truncates toward zero, so a negative
// remainder takes + 2 pi
__device__ inline float pendulum_angle_normalize(float x) {
  float r = fmodf(x + PEND_PI, PEND_2PI);
  r = r < 0.f ? r + PEND_2PI : r;
  return r - PEND_PI;
}
__device__ inline float pendulum_wrap(float th) {
  return th >= PEND_PI ? th - PEND_2PI : (th < -PEND_PI ? th + PEND_2PI : th);
}
// The step in two halves, as CartPole's: the action-independent terms (pendulum_pre: the gravity term 3 g / (2 l) sin th and
// the cost's angle_normalize(th)^2 + 0.1 thdot^2) and the rest (pendulum_post: the torque clip, the action's cost, the
// integration, the speed clip, the wrap and the new angle's cos / sin).  Explicit fmaf: every route runs exactly these
// operations whatever the compiler would contract.
struct PendulumPre {
  float grav, cost0;  // 15 sin th, angle_normalize(th)^2 + 0.1 thdot^2
};
__device__ inline PendulumPre pendulum_pre(float th, float thdot) {
  const float an = pendulum_angle_normalize(th);
  PendulumPre p;
  p.grav = 15.0f * sinf(th);
  p.cost0 = fmaf(0.1f * thdot, thdot, an * an);
  return p;
}
// s = {th, thdot} in / out; returns the reward, writes the observation (cos th', sin th', thdot')
__device__ inline float pendulum_post(const PendulumPre& p, float (&s)[2], float action, float (&obs)[3]) {
  const float u = fminf(fmaxf(action, -2.0f), 2.0f);
  const float cost = fmaf(0.001f * u, u, p.cost0);
  const float acc = fmaf(3.0f, u, p.grav);
  const float thdot = fminf(fmaxf(fmaf(acc, 0.05f, s[1]), -8.0f), 8.0f);
  const float th = pendulum_wrap(fmaf(thdot, 0.05f, s[0]));
  float sn, cs;
  sincosf(th, &sn, &cs);
  s[0] = th; s[1] = thdot;
  obs[0] = cs; obs[1] = sn; obs[2] = thdot;
  return -cost;
}
__device__ inline void pendulum_obs(const float (&s)[2], float* __restrict__ obs) {
  float sn, cs;
  sincosf(s[0], &sn, &cs);
  obs[0] = cs; obs[1] = sn; obs[2] = s[1];
}

// --------------------------------------------------------------------------------------------------
// Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0 (gymnasium classic_control acrobot.py / mountain_car.py /
// continuous_mountain_car.py) in fp32: Discrete(3) actions, MountainCarContinuous a Box(-1, 1, (1,)) force.
//
// Written for reproducible arithmetic in translation units built with -ffast-math (orl_act.hip): the functions below turn
// off reassociation and implicit contraction (ORL_CC_FP_EXACT - every fused multiply-add is an explicit fmaf), and the
// trigonometry calls the device library's accurate sin / cos / sincos (__ocml_*_f32: what sinf / cosf / sincosf are
// without -ffast-math; with it the header maps sinf / cosf to the __sinf / __cosf hardware approximations).  Divisions
// are the translation unit's (-ffast-math: a correctly scaled reciprocal and a product, within 1 ulp of IEEE).  So an env
// steps through the same operations, bit for bit, wherever it is inlined.
//
// Deviations from gymnasium, both for Acrobot:
//   * fp32 instead of float64 (gymnasium's np.append promotes the state to float64);
//   * cos(x - pi/2) is written as sin(x) (equal in real arithmetic), and the unit masses / lengths / inertias are folded
//     into the constants of _dsdt (d1 = 3.5 + cos th2, d2 = 1.25 + 0.5 cos th2, d2^2 / d1 = d2 (d2 / d1)).
// And one for MountainCarContinuous:
//   * fp32 instead of float64 for the step and the reward (gymnasium steps in float64 and rounds the state to float32
//     after every step, so only the step's intermediate values and the reward differ).
// The wrap of th1 / th2 into [-pi, pi] is gymnasium's while loop, bounded at 16 turns each way: the states reachable in a
// step (|th| <= pi + dt |dth| with the bounded speeds and RK4's intermediate ones) never need more than a few.
// Reset states come from the engine's own Philox stream keyed (seed, env, episode), as CartPole's do (each env under its
// own key).
// --------------------------------------------------------------------------------------------------
constexpr int ACROBOT_STATE_W = 6;      // {th1, th2, dth1, dth2, steps_in_episode, episodes}
constexpr int MOUNTAINCAR_STATE_W = 4;  // {position, velocity, steps_in_episode, episodes}
// at the start of every function body below: no reassociation, no contraction but the explicit fmaf
#define ORL_CC_FP_EXACT _Pragma("clang fp reassociate(off) contract(off)")
constexpr float ACRO_PI = 3.14159265358979323846f, ACRO_2PI = 6.28318530718f;
constexpr float ACRO_MAX_VEL_1 = 4.0f * 3.14159265358979323846f, ACRO_MAX_VEL_2 = 9.0f * 3.14159265358979323846f;
__device__ inline float cc_sin(float x) { return __ocml_sin_f32(x); }
__device__ inline float cc_cos(float x) { return __ocml_cos_f32(x); }
__device__ inline void cc_sincos(float x, float& s, float& c) {
  float ct;
  s = __ocml_sincos_f32(x, (__attribute__((opencl_private)) float*)&ct);
  c = ct;
}
__device__ inline void acrobot_reset(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[4]) {
  ORL_CC_FP_EXACT
  const u4 r = philox4x32_10(seed, env, 0xAC40B000u, episode, 0u);
  s[0] = fmaf(u01(r.x), 0.2f, -0.1f);
  s[1] = fmaf(u01(r.y), 0.2f, -0.1f);
  s[2] = fmaf(u01(r.z), 0.2f, -0.1f);
  s[3] = fmaf(u01(r.w), 0.2f, -0.1f);
}
// _dsdt (book dynamics) of state s under torque a: returns (dth1, dth2, ddth1, ddth2)
__device__ inline void acrobot_dsdt(const float (&s)[4], float a, float (&ds)[4]) {
  ORL_CC_FP_EXACT
  float s2, c2;
  cc_sincos(s[1], s2, c2);
  const float s1 = cc_sin(s[0]);
  const float s12 = cc_sin(s[0] + s[1]);
  const float d1 = 3.5f + c2;
  const float d2 = fmaf(0.5f, c2, 1.25f);
  const float phi2 = 4.9f * s12;
  const float w = fmaf(s[3], s[3], (2.0f * s[3]) * s[2]);  // dth2^2 + 2 dth2 dth1
  const float phi1 = fmaf(-0.5f * s2, w, fmaf(14.7f, s1, phi2));
  const float r = d2 / d1;
  const float num = fmaf(-0.5f * s2, s[2] * s[2], fmaf(r, phi1, a)) - phi2;
  const float dd2 = num / fmaf(-d2, r, 1.25f);
  const float dd1 = -fmaf(d2, dd2, phi1) / d1;
  ds[0] = s[2]; ds[1] = s[3]; ds[2] = dd1; ds[3] = dd2;
}
__device__ inline float acrobot_wrap(float x) {
  ORL_CC_FP_EXACT
#pragma unroll 1
  for (int i = 0; i < 16 && x > ACRO_PI; ++i) x = x - ACRO_2PI;
#pragma unroll 1
  for (int i = 0; i < 16 && x < -ACRO_PI; ++i) x = x + ACRO_2PI;
  return x;
}
// One step of state s (in / out) under action a in {0, 1, 2} (torque a - 1): rk4 over [0, dt], the wrap, the speed bounds;
// writes the observation (cos th1, sin th1, cos th2, sin th2, dth1, dth2) and returns whether the new state is terminal.
__device__ inline bool acrobot_step(float (&s)[4], int a, float (&obs)[6]) {
  ORL_CC_FP_EXACT
  const float torque = (float)(a - 1), dt = 0.2f, dt2 = 0.1f, dt6 = 0.2f / 6.0f;
  float k1[4], k2[4], k3[4], k4[4], y[4];
  acrobot_dsdt(s, torque, k1);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaf(dt2, k1[i], s[i]);
  acrobot_dsdt(y, torque, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaf(dt2, k2[i], s[i]);
  acrobot_dsdt(y, torque, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaf(dt, k3[i], s[i]);
  acrobot_dsdt(y, torque, k4);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaf(dt6, fmaf(2.0f, k3[i], fmaf(2.0f, k2[i], k1[i])) + k4[i], s[i]);
  s[0] = acrobot_wrap(y[0]);
  s[1] = acrobot_wrap(y[1]);
  s[2] = fminf(fmaxf(y[2], -ACRO_MAX_VEL_1), ACRO_MAX_VEL_1);
  s[3] = fminf(fmaxf(y[3], -ACRO_MAX_VEL_2), ACRO_MAX_VEL_2);
  float sn1, cs1, sn2, cs2;
  cc_sincos(s[0], sn1, cs1);
  cc_sincos(s[1], sn2, cs2);
  obs[0] = cs1; obs[1] = sn1; obs[2] = cs2; obs[3] = sn2; obs[4] = s[2]; obs[5] = s[3];
  return -cs1 - cc_cos(s[1] + s[0]) > 1.0f;
}
__device__ inline void acrobot_obs(const float (&s)[4], float (&obs)[6]) {
  float sn1, cs1, sn2, cs2;
  cc_sincos(s[0], sn1, cs1);
  cc_sincos(s[1], sn2, cs2);
  obs[0] = cs1; obs[1] = sn1; obs[2] = cs2; obs[3] = sn2; obs[4] = s[2]; obs[5] = s[3];
}

// MountainCar-v0: position p ~ U(-0.6, -0.4), velocity 0 at reset.  The step in two halves, as CartPole's: the gravity
// term cos(3 p) (-0.0025) does not depend on the action (mountaincar_pre), the rest does (mountaincar_post).
__device__ inline void mountaincar_reset(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[2]) {
  ORL_CC_FP_EXACT
  const u4 r = philox4x32_10(seed, env, 0x3C4A0000u, episode, 0u);
  s[0] = fmaf(u01(r.x), 0.2f, -0.6f);
  s[1] = 0.0f;
}
__device__ inline float mountaincar_pre(float p) {
  ORL_CC_FP_EXACT
  return cc_cos(3.0f * p) * -0.0025f; }
// s = {p, v} in / out; returns whether the new state is terminal (the reward is -1 on every step)
__device__ inline bool mountaincar_post(float (&s)[2], float pre, int a) {
  ORL_CC_FP_EXACT
  float v = s[1] + fmaf((float)(a - 1), 0.001f, pre);
  v = fminf(fmaxf(v, -0.07f), 0.07f);
  float p = s[0] + v;
  p = fminf(fmaxf(p, -1.2f), 0.6f);
  if (p == -1.2f && v < 0.0f) v = 0.0f;
  s[0] = p; s[1] = v;
  return p >= 0.5f && v >= 0.0f;
}
// MountainCarContinuous-v0 (gymnasium classic_control continuous_mountain_car.py): the same car and hill, a Box(-1, 1, (1,))
// force of power 0.0015, the goal at 0.45 (not MountainCar-v0's 0.5), reward -0.1 a^2 on every step plus 100 on the terminal
// one - charged on the UNCLIPPED action a (gymnasium's math.pow(action[0], 2)), while the dynamics use the clipped force.
// The gravity term is mountaincar_pre's.  The deviations are those listed above (fp32, the accurate cos, the Philox resets).
constexpr int MOUNTAINCAR_CONT_STATE_W = 4;  // {position, velocity, steps_in_episode, episodes}
__device__ inline void mountaincar_cont_reset(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[2]) {
  ORL_CC_FP_EXACT
  const u4 r = philox4x32_10(seed, env, 0x3CC40000u, episode, 0u);
  s[0] = fmaf(u01(r.x), 0.2f, -0.6f);
  s[1] = 0.0f;
}
// s = {p, v} in / out, pre = mountaincar_pre(p), action unclipped; returns whether the new state is terminal
__device__ inline bool mountaincar_cont_post(float (&s)[2], float pre, float action) {
  ORL_CC_FP_EXACT
  const float force = fminf(fmaxf(action, -1.0f), 1.0f);
  float v = s[1] + fmaf(force, 0.0015f, pre);
  v = fminf(fmaxf(v, -0.07f), 0.07f);
  float p = s[0] + v;
  p = fminf(fmaxf(p, -1.2f), 0.6f);
  if (p == -1.2f && v < 0.0f) v = 0.0f;
  s[0] = p; s[1] = v;
  return p >= 0.45f && v >= 0.0f;
}
__device__ inline float mountaincar_cont_reward(bool term, float action) {
  ORL_CC_FP_EXACT
  return (term ? 100.0f : 0.0f) - (action * action) * 0.1f;
}
// actions of the Discrete(3) envs as a class index: the float action is truncated and clamped into {0, 1, 2}
__device__ inline int discrete3_action(float action) {
  const int a = (int)action;
  return a < 0 ? 0 : (a > 2 ? 2 : a);
}

// One env.step of env `n` at global time `tg` on the env's state row `st` / episode statistics `e` (register or memory
// copies): writes the next observation to obs_out[0..D), returns the reward and whether the episode ended.  The one
// definition of the envs' arithmetic: every route steps through it.
template <int ENV>
__device__ inline void env_step_state(float* __restrict__ st, float* __restrict__ e, int n, int D, uint64_t seed,
                                      int episode_limit, uint64_t tg, float action, float* __restrict__ obs_out, float& r,
                                      bool& d) {
  if (ENV == ORL_ENV_SYNTH) {
    r = synth_reward(seed, (uint32_t)n, tg);
    const float c = st[0] + 1.f;
    d = c >= (float)episode_limit;
    st[0] = d ? 0.f : c;
    for (int b = 0; b < (D + 3) / 4; ++b) {
      float o[4];
      synth_obs_block(seed, (uint32_t)n, tg + 1, (uint32_t)b, o);
      for (int k = 0; k < 4; ++k)
        if (4 * b + k < D) obs_out[4 * b + k] = o[k];
    }
  } else if (ENV == ORL_ENV_PENDULUM) {
    float s[2] = {st[0], st[1]};
    const PendulumPre p = pendulum_pre(s[0], s[1]);
    float o[3];
    r = pendulum_post(p, s, action, o);
    const float steps = st[2] + 1.f;
    d = steps >= (float)episode_limit;  // never terminates: truncation only (done = terminated or truncated, no bootstrap)
    st[2] = d ? 0.f : steps;
    if (d) {
      st[3] += 1.f;
      pendulum_reset(seed, (uint32_t)n, (uint32_t)st[3], s);  // auto-reset: the first observation of the next episode
      pendulum_obs(s, o);
    }
    st[0] = s[0]; st[1] = s[1];
    for (int k = 0; k < 3; ++k) obs_out[k] = o[k];
  } else if (ENV == ORL_ENV_ACROBOT) {
    float s[4] = {st[0], st[1], st[2], st[3]}, o[6];
    const bool term = acrobot_step(s, discrete3_action(action), o);
    const float steps = st[4] + 1.f;
    d = term || steps >= (float)episode_limit;
    r = term ? 0.f : -1.f;
    st[4] = d ? 0.f : steps;
    if (d) {
      st[5] += 1.f;
      acrobot_reset(seed, (uint32_t)n, (uint32_t)st[5], s);  // auto-reset: the first observation of the next episode
      acrobot_obs(s, o);
    }
    for (int k = 0; k < 4; ++k) st[k] = s[k];
    for (int k = 0; k < 6; ++k) obs_out[k] = o[k];
  } else if (ENV == ORL_ENV_MOUNTAINCAR) {
    float s[2] = {st[0], st[1]};
    const bool term = mountaincar_post(s, mountaincar_pre(s[0]), discrete3_action(action));
    const float steps = st[2] + 1.f;
    d = term || steps >= (float)episode_limit;
    r = -1.f;
    st[2] = d ? 0.f : steps;
    if (d) {
      st[3] += 1.f;
      mountaincar_reset(seed, (uint32_t)n, (uint32_t)st[3], s);
    }
    st[0] = s[0]; st[1] = s[1];
    obs_out[0] = s[0]; obs_out[1] = s[1];
  } else if (ENV == ORL_ENV_MOUNTAINCAR_CONT) {
    float s[2] = {st[0], st[1]};
    const bool term = mountaincar_cont_post(s, mountaincar_pre(s[0]), action);
    r = mountaincar_cont_reward(term, action);
    const float steps = st[2] + 1.f;
    d = term || steps >= (float)episode_limit;
    st[2] = d ? 0.f : steps;
    if (d) {
      st[3] += 1.f;
      mountaincar_cont_reset(seed, (uint32_t)n, (uint32_t)st[3], s);
    }
    st[0] = s[0]; st[1] = s[1];
    obs_out[0] = s[0]; obs_out[1] = s[1];
  } else {
    float s[4] = {st[0], st[1], st[2], st[3]};
    const bool term = cartpole_step(s, (int)action);
    const float steps = st[4] + 1.f;
    d = term || steps >= (float)episode_limit;
    r = 1.0f;
    st[4] = d ? 0.f : steps;
    if (d) {
      st[5] += 1.f;
      cartpole_reset(seed, (uint32_t)n, (uint32_t)st[5], s);
    }
    for (int k = 0; k < 4; ++k) { st[k] = s[k]; obs_out[k] = s[k]; }
  }
  if (e != nullptr) {
    e[0] += r; e[1] += 1.f;
    if (d) { e[2] += e[0]; e[3] += 1.f; e[0] = 0.f; e[1] = 0.f; }
  }
}

// the same on the state arrays in memory (the stand-alone env_step_kernel's body)
template <int ENV>
__device__ inline void env_step_one(float* __restrict__ env_state, float* __restrict__ ep_stats, int n, int D,
                                    uint64_t seed, int episode_limit, uint64_t tg, float action,
                                    float* __restrict__ obs_out, float& r, bool& d) {
  constexpr int W = ENV == ORL_ENV_SYNTH         ? SYNTH_STATE_W
                    : ENV == ORL_ENV_PENDULUM    ? PENDULUM_STATE_W
                    : ENV == ORL_ENV_ACROBOT     ? ACROBOT_STATE_W
                    : ENV == ORL_ENV_MOUNTAINCAR ? MOUNTAINCAR_STATE_W
                    : ENV == ORL_ENV_MOUNTAINCAR_CONT ? MOUNTAINCAR_CONT_STATE_W
                                                 : CARTPOLE_STATE_W;
  env_step_state<ENV>(env_state + (size_t)n * W, ep_stats != nullptr ? ep_stats + (size_t)n * 4 : nullptr, n, D, seed,
                      episode_limit, tg, action, obs_out, r, d);
}

}  // namespace orl
