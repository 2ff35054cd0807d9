// tg_stack_test.hip - libtactile_gym_hip_test.so: the frame-stack launchers on raw device buffers (tg_selftest_stack).  TEST INFRASTRUCTURE
// (include/tactile_gym_hip_test.h): linked with the product's own tg_stack.o, so launch_frame_stack, launch_obs_stack, k_frame_stack and
// k_obs_stack are the product's; tests/test_gpu_stack_matrix.py calls it.  It copies the description into StackArgs / VisStack and returns the
// launcher's return value: no checks of its own, no allocation, no synchronisation.
#include "../../include/tactile_gym_hip_test.h"
#include "tg_stack.h"

extern "C" int tg_selftest_stack(const tg_stack_test* t, void* stream) {
    if (!t) return -1;
    tg::StackArgs a;
    a.num_envs = t->num_envs; a.H = t->H; a.W = t->W; a.n = t->n; a.mode = t->mode; a.rewrite_all = t->rewrite_all;
    a.flag = t->flag; a.frame = t->frame; a.term_frame = t->term_frame; a.tmpl = t->tmpl;
    a.stack = t->stack; a.term_stack = t->term_stack; a.rec = t->rec;
    for (int k = 0; k < 2; ++k) {
        a.vec[k].src = t->vec[k].src; a.vec[k].term = t->vec[k].term; a.vec[k].stack = t->vec[k].stack; a.vec[k].term_stack = t->vec[k].term_stack;
        a.vec[k].dim = t->vec[k].dim; a.vec[k].pitch = t->vec[k].pitch;
    }
    if (t->which == TG_STACK_TEST_FRAME) return tg::launch_frame_stack(a, (hipStream_t)stream);
    tg::VisStack v;
    v.frame = t->vis_frame; v.term_frame = t->vis_term_frame; v.stack = t->vis_stack; v.term_stack = t->vis_term_stack;
    v.H = t->vis_H; v.W = t->vis_W;
    return tg::launch_obs_stack(a, v, t->channels_first, (hipStream_t)stream);
}
