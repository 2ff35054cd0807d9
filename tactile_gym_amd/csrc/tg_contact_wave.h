// tg_contact_wave.h - launch interface of the wave-per-env contact solver (tg_contact_wave.hip).
//
// Every launcher has a side-effect-free can_run_* predicate beside it: which combinations are instantiated, and their LDS and hull limits, is
// known in tg_contact_wave.hip only.  tg_create asks the predicates once when it chooses the context's step family (tg_api.hip:
// choose_step_plan); a configuration a predicate refuses is a lane-per-env context from the start.  The launchers ask the same predicate and
// return 0, or -3 without launching: the caller has picked a family that cannot run, which tg_step / tg_reset report as an internal error.
#pragma once
#include <hip/hip_runtime.h>

namespace tg {

struct State;

// object_push (env_kind TG_ENV_OBJECT_PUSH; UR5 and MG400) / object_roll (TG_ENV_OBJECT_ROLL; UR5): f64, cone friction, the tip core's hull
// (n_tip_verts vertices) staged in LDS.  One answer for the step and the reset: an env never changes mapping between the two.
bool can_run_contact_wave(int env_kind, int physics_dtype, int topology, int cone_friction, int n_tip_verts, int narrowphase);
// Enqueue one env step on `stream` with the wave-per-env mapping: one 64-lane wavefront per env, one solver row per lane.  d_robot / d_const:
// DevRobot<T> / EnvConst<T> of the context (T by physics_dtype).
int launch_step_contact_wave(int env_kind, int physics_dtype, int topology, int control_mode, int cone_friction, int num_envs, int n_tip_verts,
                             hipStream_t stream,
                             const void* d_robot, const void* d_const, const State& st, const float* d_actions, int narrowphase = 0);
// narrowphase (tg_config.narrowphase, object_push, f64): 0 closed forms; otherwise the tip - cube pair goes through GJK / EPA and the persistent
// manifold (tg_narrowphase.hpp): the kernel's four-tip-slot variant.
// env.reset() for the envs flagged in d_mask (nullptr: all) with the same mapping: one wavefront per resetting env, the others exit at once.
int launch_reset_contact_wave(int env_kind, int physics_dtype, int topology, int cone_friction, int num_envs, int n_tip_verts, hipStream_t stream,
                              const void* d_robot, const void* d_const, const State& st, const uint8_t* d_mask, int narrowphase = 0);

// object_balance (arm + pole + point-to-point constraint), TCP_velocity_control, f64, UR5: one wavefront per env (the env's own licence for the
// analytic fixed point, full ticks on the wave mapping).  inline_reset: finished envs are reset by their own wavefront at the end of the step
// (the template-only reset: the caller has made sure the template is valid) - no k_reset_body launch behind this one.
bool can_run_body_wave(int physics_dtype, int topology, int control_mode);
int launch_step_body_wave(int physics_dtype, int topology, int control_mode, int num_envs, hipStream_t stream, const void* d_robot, const void* d_const,
                          const State& st, const float* d_actions, int inline_reset);
// edge_follow / surface_follow (contact-free arm, TCP_velocity_control, f64; UR5 and MG400): one wavefront per env, every tick a full tick
// (lane-parallel dynamics, the motor pass as a linear map).
bool can_run_arm_wave(int physics_dtype, int control_mode);
int launch_step_arm_wave(int physics_dtype, int topology, int control_mode, int num_envs, hipStream_t stream, const void* d_robot, const void* d_const,
                         const State& st, const float* d_actions);

}  // namespace tg
