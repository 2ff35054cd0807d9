// tg_spin.h - launch interface of object_balance's spinning_plate step (tg_spin.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace tg {

struct State;

// One env step of object_balance with object_mode "spinning_plate" on `stream`: one wavefront per env (f64, UR5 chain).  n_dish: hull vertices of
// the dish (staged in LDS; the spool's ride on the lanes).  can_run_spin: whether the combination is instantiated (side-effect free; tg_create
// refuses a spinning_plate context it is false for - there is no other mapping).  The launcher returns 0, or -3 without launching when it is
// false.
bool can_run_spin(int physics_dtype, int topology, int n_dish);
int launch_step_spin(int physics_dtype, int topology, int control_mode, int num_envs, int n_dish, hipStream_t stream, const void* d_robot,
                     const void* d_const, const State& st, const float* d_actions);

}  // namespace tg
