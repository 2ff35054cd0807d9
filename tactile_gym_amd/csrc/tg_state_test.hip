// tg_state_test.hip - test entry that writes arm and free-object states into a context (include/tactile_gym_hip_test.h: tg_selftest_set_body_state),
// so that a test can start the step kernels of object_push / object_roll / object_balance anywhere, not only at the reset pose.  TEST
// INFRASTRUCTURE: linked into libtactile_gym_hip_test.so only.  No kernel of its own and nothing from the product's objects: it reads the
// context's fields through tg_ctx.hpp and copies.
#include "../../include/tactile_gym_hip_test.h"
#include "tg_ctx.hpp"

using namespace tg;

namespace {

// the envs the call writes: mask NULL = all
static inline bool masked(const uint8_t* mask, int i) { return mask == nullptr || mask[i] != 0; }

static bool all_finite(const double* a, int n, int k, const uint8_t* mask) {
    for (int i = 0; i < n; ++i) {
        if (!masked(mask, i)) continue;
        for (int f = 0; f < k; ++f) if (!std::isfinite(a[(size_t)i * k + f])) return false;
    }
    return true;
}
// rot: [n][stride] with the row-major matrix at offset off
static bool all_orthonormal(const double* a, int n, int stride, int off, const uint8_t* mask) {
    for (int i = 0; i < n; ++i) {
        if (!masked(mask, i)) continue;
        const double* R = a + (size_t)i * stride + off;
        for (int r = 0; r < 3; ++r)
            for (int s = 0; s < 3; ++s) {
                const double d = R[3 * r] * R[3 * s] + R[3 * r + 1] * R[3 * s + 1] + R[3 * r + 2] * R[3 * s + 2] - (r == s ? 1.0 : 0.0);
                if (!(std::fabs(d) <= 1e-9)) return false;
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det > 0.0)) return false;                       // a reflection is no orientation
    }
    return true;
}
// AoS host [n][k] -> rows row0 .. row0 + k - 1 of the SoA device array [rows][n], masked envs only (the others keep what they hold)
template <typename T> static int put_soa(tg_ctx* c, T* dev, int row0, int k, const T* host, const uint8_t* mask) {
    const int n = c->cfg.num_envs;
    std::vector<T> tmp((size_t)k * n);
    T* at = dev + (size_t)row0 * n;
    TG_HIP(hipMemcpyAsync(tmp.data(), at, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    TG_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
        if (!masked(mask, i)) continue;
        for (int f = 0; f < k; ++f) tmp[(size_t)f * n + i] = host[(size_t)i * k + f];
    }
    TG_HIP(hipMemcpyAsync(at, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    TG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
// the same value in rows row0 .. row0 + k - 1 of the masked envs
template <typename T> static int fill_soa(tg_ctx* c, T* dev, int row0, int k, T value, const uint8_t* mask) {
    std::vector<T> v((size_t)c->cfg.num_envs * k, value);
    return put_soa(c, dev, row0, k, v.data(), mask);
}

}  // namespace

extern "C" int tg_selftest_set_body_state(tg_ctx* c, const tg_body_state_test* s) {
    if (!c || !s) return fail(-1, "tg_selftest_set_body_state: NULL argument");
    const int n = c->cfg.num_envs, nd = c->robot.ndof;
    const State& st = c->st;
    const bool has_body = st.body_pos != nullptr && st.body_rot != nullptr && st.body_v != nullptr && st.body_w != nullptr;
    const bool has_goal = c->cfg.env_kind == TG_ENV_OBJECT_PUSH && st.goal_id != nullptr;
    // everything is checked before anything is written
    if ((s->body_pos || s->body_rot || s->body_linvel || s->body_angvel) && !has_body) return fail(-1, "tg_selftest_set_body_state: this env has no free body");
    if ((s->ball_pos || s->ball_linvel || s->ball_angvel) && st.ball == nullptr) return fail(-1, "tg_selftest_set_body_state: this env has no ball");
    if (s->dish_state && st.dish == nullptr) return fail(-1, "tg_selftest_set_body_state: this env has no dish");
    if (s->goal_id && !has_goal) return fail(-1, "tg_selftest_set_body_state: this env has no goal trajectory");
    const struct { const double* p; int k; } reals[] = {{s->q, nd}, {s->qd, nd}, {s->body_pos, 3}, {s->body_rot, 9}, {s->body_linvel, 3}, {s->body_angvel, 3},
                                                        {s->ball_pos, 3}, {s->ball_linvel, 3}, {s->ball_angvel, 3}, {s->dish_state, 18}};
    for (const auto& r : reals)
        if (r.p && !all_finite(r.p, n, r.k, s->mask)) return fail(-1, "tg_selftest_set_body_state: a value is not finite");
    if (s->body_rot && !all_orthonormal(s->body_rot, n, 9, 0, s->mask)) return fail(-1, "tg_selftest_set_body_state: body_rot is not a rotation (1e-9)");
    if (s->dish_state && !all_orthonormal(s->dish_state, n, 18, 3, s->mask)) return fail(-1, "tg_selftest_set_body_state: the dish's rotation is not a rotation (1e-9)");
    if (s->goal_id)
        for (int i = 0; i < n; ++i)
            if (masked(s->mask, i) && (s->goal_id[i] < 0 || s->goal_id[i] > c->cfg.traj_n_points)) return fail(-1, "tg_selftest_set_body_state: goal_id outside [0, traj_n]");
    TG_ENTER(c);
    TG_HIP(hipStreamSynchronize(c->stream));
    int rc = 0;
    // the given fields, AoS -> the context's SoA arrays
    if (s->q && (rc = put_soa(c, st.q, 0, nd, s->q, s->mask))) return rc;
    if (s->qd && (rc = put_soa(c, st.qd, 0, nd, s->qd, s->mask))) return rc;
    if (s->body_pos && (rc = put_soa(c, st.body_pos, 0, 3, s->body_pos, s->mask))) return rc;
    if (s->body_rot && (rc = put_soa(c, st.body_rot, 0, 9, s->body_rot, s->mask))) return rc;
    if (s->body_linvel && (rc = put_soa(c, st.body_v, 0, 3, s->body_linvel, s->mask))) return rc;
    if (s->body_angvel && (rc = put_soa(c, st.body_w, 0, 3, s->body_angvel, s->mask))) return rc;
    if (s->ball_pos && (rc = put_soa(c, st.ball, 0, 3, s->ball_pos, s->mask))) return rc;
    if (s->ball_linvel && (rc = put_soa(c, st.ball, 3, 3, s->ball_linvel, s->mask))) return rc;
    if (s->ball_angvel && (rc = put_soa(c, st.ball, 6, 3, s->ball_angvel, s->mask))) return rc;
    if (s->dish_state && (rc = put_soa(c, st.dish, 0, 18, s->dish_state, s->mask))) return rc;
    if (s->goal_id && (rc = put_soa(c, st.goal_id, 0, 1, s->goal_id, s->mask))) return rc;
    // what a teleport clears: the solver licence (a new configuration: full solve and exact sines / cosines next), the one-shot force / torque of
    // the last reset (one flag for the pole's force, the ball's torque and the dish's force and torque; the ball's torque itself), the cached
    // contact points (the count of the tip - cube manifold, of the dish - spool manifold), the contact pairs of the last tick
    if ((rc = fill_soa<int32_t>(c, st.licence, 0, 1, 0, s->mask))) return rc;
    if (st.ext_pending && (rc = fill_soa<uint8_t>(c, st.ext_pending, 0, 1, 0, s->mask))) return rc;
    if (st.ball && (rc = fill_soa<double>(c, st.ball, 9, 3, 0.0, s->mask))) return rc;
    if (st.mani && (rc = fill_soa<double>(c, st.mani, 36, 1, 0.0, s->mask))) return rc;
    if (st.contact_code && (rc = fill_soa<int32_t>(c, st.contact_code, 0, 1, 0, s->mask))) return rc;
    TG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// State.reset_tmpl as the reset kernels left it.  Its size is the allocation's (tg_kernels.hpp: kPushTmplWords, kBodyTmplWords).
extern "C" int tg_selftest_get_reset_template(tg_ctx* c, double* out, int32_t cap, int32_t* n_words) {
    if (!c || !n_words) return fail(-1, "tg_selftest_get_reset_template: NULL argument");
    *n_words = 0;
    if (c->st.reset_tmpl == nullptr) return fail(-1, "tg_selftest_get_reset_template: this context has no reset template");
    const int words = c->cfg.env_kind == TG_ENV_OBJECT_PUSH ? kPushTmplWords : kBodyTmplWords;
    *n_words = words;
    if (!out || cap < words) return fail(-1, "tg_selftest_get_reset_template: out holds fewer than *n_words doubles");
    TG_ENTER(c);
    TG_HIP(hipStreamSynchronize(c->stream));
    TG_HIP(hipMemcpyAsync(out, c->st.reset_tmpl, (size_t)words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
