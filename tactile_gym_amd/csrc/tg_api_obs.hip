// tg_api_obs.hip - the C ABI's observation side (include/tactile_gym_hip.h): where every observation buffer lives and how wide a row of it is
// (resolve, the one table: DESIGN.md 4.20), the entries that hand a buffer out or copy it to the host, the render targets, the frame stack and the
// observation layout (their allocation here, their kernels in tg_stack.hip).  Names no kernel: the oracle vectors are drawn by tg_api.hip's
// oracle_draw (tg_ctx.hpp).
#include "tg_ctx.hpp"

namespace tg {

static int feature_dim(const tg_ctx* c) { return c->cfg.env_kind == TG_ENV_OBJECT_ROLL ? 3 : c->cfg.env_kind == TG_ENV_SURFACE_FOLLOW_AUTO ? 6 : 12; }
// the observation_mode "oracle" vectors [n][34], allocated on first use (zeroed)
static int need_oracle(tg_ctx* c, float*& buf) { return buf ? 0 : dev_alloc(c, buf, (size_t)c->cfg.num_envs * 34 * sizeof(float)); }

// Where observation `key` (TG_OBS_KEY_*) lives and how many bytes one env's row of it has: the current or the terminal one, plain or stacked
// (what tg_get_obs_stack hands out).  The only place that spells a key's precondition, its buffers and its row; a refusal is -1 with the
// text the entries have always given - the plain ones under the entry's name `who`, the stacked ones bare.
//   key      plain buffer (current / terminal)        row           stacked buffer                      row                  needs
//   tactile  obs_buf(c) / d_term                      H W           d_stack / d_stack_term              H W n                -
//            (stacked with n = 1, channels first: [n][1][H][W] is the plain buffer itself)
//   visual   d_vis / d_vis_term                       3 H W         d_vstack / d_vstack_term            3 H W n              plain: a scene; stacked: a visual stack
//   oracle   d_oracle / d_oracle_term                 4 dim         d_stack_vec[0] / d_stack_vec_term   4 dim n              terminal or stacked: tg_enable_oracle_obs
//            (plain and current: allocated on first use, and drawn here unless every step draws it)
//   feature  st.feature / st.term_feature             4 * 12        d_stack_vec[1] / d_stack_vec_term   4 feature_dim n      an env with extended_feature
// A stacked key other than visual (drawn by the scene camera, stacked under channels first at n = 1 too) needs n > 1, and is asked that first.
struct ObsBuf { void* p = nullptr; size_t row = 0; };
static int resolve(tg_ctx* c, int32_t key, int32_t terminal, bool stacked, const char* who, ObsBuf& b) {
    const auto refuse = [&](const char* msg) { return fail(-1, stacked ? std::string(msg) : std::string(who) + ": " + msg); };
    const auto pick = [&](void* cur, void* term) { b.p = terminal ? term : cur; };
    if (stacked && key != TG_OBS_KEY_VISUAL && c->stack_n <= 1 && !(key == TG_OBS_KEY_TACTILE && c->obs_cf)) return refuse("no frame stack (tg_set_frame_stack n > 1)");
    const size_t n = stacked ? c->stack_n : 1;
    switch (key) {
        case TG_OBS_KEY_TACTILE:
            if (n > 1) pick(c->d_stack, c->d_stack_term); else pick(obs_buf(c), c->d_term);
            b.row = (size_t)c->H * c->W * n;
            return 0;
        case TG_OBS_KEY_VISUAL:
            if (stacked && !c->d_vstack) return refuse("no visual stack (a scene drawn every step, with tg_set_frame_stack n > 1 or tg_set_obs_layout 1)");
            if (!stacked && !c->scene_on) return refuse("no scene (tg_set_scene)");
            if (stacked) pick(c->d_vstack, c->d_vstack_term); else pick(c->d_vis, c->d_vis_term);
            b.row = (size_t)c->scene.H * c->scene.W * 3 * n;
            return 0;
        case TG_OBS_KEY_ORACLE:
            if ((stacked || terminal) && !c->oracle_every_step)
                return refuse(stacked ? "no stacked oracle observation (tg_enable_oracle_obs before tg_set_frame_stack)" : "needs tg_enable_oracle_obs");
            if (!stacked && !terminal) {
                if (int rc = need_oracle(c, c->d_oracle)) return rc;
                if (!c->oracle_every_step) oracle_draw(c, c->d_oracle);     // (enabled: tg_step / tg_reset have already written it)
                TG_HIP(hipGetLastError());
            }
            if (stacked) pick(c->d_stack_vec[0], c->d_stack_vec_term[0]); else pick(c->d_oracle, c->d_oracle_term);
            b.row = (size_t)oracle_dim(c) * n * sizeof(float);
            return 0;
        case TG_OBS_KEY_FEATURE:
            if (!env_has_feature(c->cfg.env_kind)) return refuse("this env has no extended_feature observation");
            if (stacked) pick(c->d_stack_vec[1], c->d_stack_vec_term[1]); else pick(c->st.feature, c->st.term_feature);
            b.row = (stacked ? feature_dim(c) * n : 12) * sizeof(float);     // (the plain rows are 12 floats wide in every env)
            return 0;
    }
    return refuse("unknown observation key");
}

// The frame stack's update after a step (flag = st.done) or a reset (flag = the reset mask, null: every env); tg_stack.hip.  Reads the finished
// observation buffers of that step / reset, so it is the last launch of the sequence.  It names the table's buffers once more, all of them in one
// argument block: it runs in every step, where a refusal has no place and a string no time.
static bool stack_rewrite_all() {
    static const bool on = [] { const char* e = getenv("TG_STACK_REWRITE_ALL"); return e && e[0] == '1'; }();   // read once per process
    return on;
}
int stack_update(tg_ctx* c, int mode, const uint8_t* flag) {
    if (c->stack_n <= 1 && !c->d_vstack) return 0;
    StackArgs a;
    a.num_envs = c->cfg.num_envs; a.H = c->H; a.W = c->W; a.n = c->stack_n; a.mode = mode; a.rewrite_all = stack_rewrite_all() ? 1 : 0;
    a.flag = flag;
    const bool term = mode == kStackStep && c->cfg.auto_reset;
    a.frame = c->d_obs; a.term_frame = c->d_term; a.tmpl = c->d_tile_tmpl; a.stack = c->d_stack; a.rec = c->d_stack_rec;   // (a stack, or channels first: no render targets, obs_buf(c) is d_obs)
    a.term_stack = term ? c->d_stack_term : nullptr;
    for (int k = 0; k < 2; ++k) {
        if (!c->d_stack_vec[k]) continue;
        StackVec& v = a.vec[k];
        v.dim = c->stack_vec_dim[k];
        v.pitch = k == 0 ? v.dim : 12;
        v.src = k == 0 ? c->d_oracle : c->st.feature;
        v.term = k == 0 ? c->d_oracle_term : c->st.term_feature;
        v.stack = c->d_stack_vec[k];
        v.term_stack = term ? c->d_stack_vec_term[k] : nullptr;
    }
    if (!c->d_vstack && !c->obs_cf) {
        if (launch_frame_stack(a, c->stream) != 0) return fail(-2, "frame stack launch failed");
        return 0;
    }
    if (c->stack_n <= 1) a.frame = nullptr;     // channels first, n = 1: the tactile buffer is its own stack
    VisStack v;
    if (c->d_vstack) {
        v.frame = c->d_vis; v.term_frame = c->d_vis_term; v.stack = c->d_vstack; v.term_stack = term ? c->d_vstack_term : nullptr;
        v.H = c->scene.H; v.W = c->scene.W;
    }
    if (launch_obs_stack(a, v, c->obs_cf, c->stream) != 0) return fail(-2, "observation stack launch failed");
    return 0;
}

// ---- the two ways to the host
static int copy_batch(tg_ctx* c, const ObsBuf& b, void* dst) {
    TG_HIP(hipMemcpyAsync(dst, b.p, b.row * c->cfg.num_envs, hipMemcpyDeviceToHost, c->stream));
    TG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
// the rows of the envs `env_ids`, in that order
static int copy_rows(tg_ctx* c, const ObsBuf& b, const int32_t* env_ids, int32_t count, void* dst, const char* who) {
    for (int32_t k = 0; k < count; ++k)
        if (env_ids[k] < 0 || env_ids[k] >= c->cfg.num_envs) return fail(-1, std::string(who) + ": env id out of range");
    // through a pinned staging block (64 rows at a time): a device -> pageable copy of 16 KB is a staged, blocking copy of its own each time
    constexpr int kChunk = 64;
    if (count > 0 && c->h_rows_bytes < b.row * kChunk) {
        if (c->h_rows) { (void)hipHostFree(c->h_rows); c->h_rows = nullptr; c->h_rows_bytes = 0; }
        TG_HIP(hipHostMalloc((void**)&c->h_rows, b.row * kChunk, hipHostMallocDefault));
        c->h_rows_bytes = b.row * kChunk;
    }
    for (int32_t k0 = 0; k0 < count; k0 += kChunk) {
        const int32_t m = count - k0 < kChunk ? count - k0 : kChunk;
        for (int32_t k = 0; k < m; ++k)
            TG_HIP(hipMemcpyAsync(c->h_rows + (size_t)k * b.row, (const uint8_t*)b.p + (size_t)env_ids[k0 + k] * b.row, b.row, hipMemcpyDeviceToHost, c->stream));
        TG_HIP(hipStreamSynchronize(c->stream));
        memcpy((uint8_t*)dst + (size_t)k0 * b.row, c->h_rows, (size_t)m * b.row);
    }
    return 0;
}

// ---- what every tg_get_* / tg_copy_* entry below is: its own NULL arguments, TG_ENTER, resolve, hand out or copy
constexpr bool kPlain = false, kStacked = true;
static int get_entry(tg_ctx* c, int32_t key, int32_t terminal, bool stacked, const char* who, void** p) {
    if (!c || !p) return fail(-1, "NULL argument");
    TG_ENTER(c);
    ObsBuf b;
    if (int rc = resolve(c, key, terminal, stacked, who, b)) return rc;
    *p = b.p;
    return 0;
}
static int copy_entry(tg_ctx* c, int32_t key, int32_t terminal, bool stacked, const char* who, void* dst) {
    if (!c || !dst) return fail(-1, "NULL argument");
    TG_ENTER(c);
    ObsBuf b;
    if (int rc = resolve(c, key, terminal, stacked, who, b)) return rc;
    return copy_batch(c, b, dst);
}
static int rows_entry(tg_ctx* c, int32_t key, int32_t terminal, bool stacked, const char* who, const int32_t* env_ids, int32_t count, void* dst) {
    if (!c || count < 0 || (count > 0 && (!env_ids || !dst))) return fail(-1, std::string(who) + ": bad argument");
    TG_ENTER(c);
    ObsBuf b;
    if (int rc = resolve(c, key, terminal, stacked, who, b)) return rc;
    return copy_rows(c, b, env_ids, count, dst, who);
}

// ---- frame stack (VecFrameStack on the device; tg_stack.hip) ----
static void free_stack(tg_ctx* c) {
    dev_release(c, c->d_stack); dev_release(c, c->d_stack_term); dev_release(c, c->d_stack_rec); dev_release(c, c->d_vstack); dev_release(c, c->d_vstack_term);
    for (int k = 0; k < 2; ++k) { dev_release(c, c->d_stack_vec[k]); dev_release(c, c->d_stack_vec_term[k]); }
    c->stack_vec_dim[0] = c->stack_vec_dim[1] = 0;
    c->stack_n = 1;
}
// (Re)allocates every stack for n frames in layout cf, all zero.
static int alloc_stacks(tg_ctx* c, int n, int cf) {
    if (c->scene_every_step && (n > 1 || cf) && c->scene.W % 16) return fail(-1, "stacked scene images need a width that is a multiple of 16");
    TG_HIP(hipStreamSynchronize(c->stream));
    free_stack(c);
    c->obs_cf = cf;
    const size_t envs = (size_t)c->cfg.num_envs;
    if (n > 1) {
        const size_t img = envs * c->H * c->W * n, rec = envs * (c->H / 16) * (c->W / 16);   // (the same bytes in either layout)
        if (dev_alloc(c, c->d_stack, img) || dev_alloc(c, c->d_stack_term, img) || dev_alloc(c, c->d_stack_rec, rec)) return -2;   // rec 0: no slot holds the template, the first update writes every block
        c->stack_vec_dim[0] = c->oracle_every_step ? oracle_dim(c) : 0;
        c->stack_vec_dim[1] = env_has_feature(c->cfg.env_kind) ? feature_dim(c) : 0;
        for (int k = 0; k < 2; ++k) {
            if (!c->stack_vec_dim[k]) continue;
            const size_t b = envs * c->stack_vec_dim[k] * n * sizeof(float);
            if (dev_alloc(c, c->d_stack_vec[k], b) || dev_alloc(c, c->d_stack_vec_term[k], b)) return -2;
        }
        c->stack_n = n;
    }
    if (c->scene_every_step && (n > 1 || cf)) {      // the visual observation modes
        const size_t b = envs * c->scene.H * c->scene.W * 3 * n;
        if (dev_alloc(c, c->d_vstack, b) || dev_alloc(c, c->d_vstack_term, b)) return -2;
    }
    TG_HIP(hipDeviceSynchronize());
    return 0;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_set_obs_targets(tg_ctx* c, int32_t count, void* const* dev_ptrs) {
    if (!c || count < 0 || count > 2 || (count > 0 && !dev_ptrs)) return fail(-1, "tg_set_obs_targets: bad argument");
    for (int k = 0; k < count; ++k) if (!dev_ptrs[k]) return fail(-1, "tg_set_obs_targets: NULL target");   // (every argument is checked before anything is changed)
    if (count > 0 && c->stack_n > 1) return fail(-1, "tg_set_obs_targets: a context with a frame stack (tg_set_frame_stack n > 1) draws into its own buffer only");
    if (count > 0 && c->obs_cf) return fail(-1, "tg_set_obs_targets: a context with channels-first observations (tg_set_obs_layout 1) draws into its own buffer only");
    TG_ENTER(c);
    TG_HIP(hipStreamSynchronize(c->stream));
    c->obs_sel = 0;
    const size_t regions = (c->rp.W % 128 == 0 && c->rp.H % 128 == 0) ? (size_t)(c->rp.W / 128) * (c->rp.H / 128) : 0;
    for (int k = 0; k < 2; ++k) {
        c->obs_ext[k] = k < count ? (uint8_t*)dev_ptrs[k] : nullptr;
        if (k < count && c->rp.drawn != nullptr && regions == 0) return fail(-3, "tg_set_obs_targets: a changed-block record without 128-pixel regions (internal)");
        if (k < count && c->rp.drawn != nullptr) {   // a changed-block record of its own: nothing in that buffer is known to hold the untouched-sensor image
            const size_t bytes = (size_t)c->cfg.num_envs * regions * 8;
            if (!c->drawn_ext[k] && dev_alloc(c, c->drawn_ext[k], bytes, kNoFill)) return -2;
            TG_HIP(hipMemset(c->drawn_ext[k], 0xFF, bytes));
        }
    }
    return 0;
}
int tg_select_obs_target(tg_ctx* c, int32_t index) {
    if (!c || index < 0 || index > 2 || (index > 0 && c->obs_ext[index - 1] == nullptr)) return fail(-1, "tg_select_obs_target: no such target");
    c->obs_sel = index;
    return 0;
}

int tg_enable_oracle_obs(tg_ctx* c) {
    if (!c) return fail(-1, "NULL ctx");
    if (c->stack_n > 1 && !c->oracle_every_step) return fail(-1, "tg_enable_oracle_obs: call it before tg_set_frame_stack");
    TG_ENTER(c);
    for (float* buf : {c->d_oracle, c->d_oracle_term})    // enabled again: the rows start from zero
        if (buf) TG_HIP(hipMemset(buf, 0, (size_t)c->cfg.num_envs * 34 * sizeof(float)));
    if (need_oracle(c, c->d_oracle) || need_oracle(c, c->d_oracle_term)) return -2;
    c->oracle_every_step = true;
    return 0;
}

int tg_get_obs_tactile(tg_ctx* c, void** p) { return get_entry(c, TG_OBS_KEY_TACTILE, 0, kPlain, "tg_get_obs_tactile", p); }
int tg_get_terminal_obs(tg_ctx* c, void** p) { return get_entry(c, TG_OBS_KEY_TACTILE, 1, kPlain, "tg_get_terminal_obs", p); }
int tg_copy_obs_tactile(tg_ctx* c, uint8_t* dst, int32_t terminal) { return copy_entry(c, TG_OBS_KEY_TACTILE, terminal, kPlain, "tg_copy_obs_tactile", dst); }
int tg_get_obs_visual(tg_ctx* c, void** p, int32_t terminal) { return get_entry(c, TG_OBS_KEY_VISUAL, terminal, kPlain, "tg_get_obs_visual", p); }
int tg_copy_obs_visual(tg_ctx* c, uint8_t* dst, int32_t terminal) { return copy_entry(c, TG_OBS_KEY_VISUAL, terminal, kPlain, "tg_copy_obs_visual", dst); }
int tg_get_obs_feature(tg_ctx* c, void** p, int32_t* dim, int32_t terminal) {
    const int rc = get_entry(c, TG_OBS_KEY_FEATURE, terminal, kPlain, "tg_get_obs_feature", p);
    if (rc == 0 && dim) *dim = 12;
    return rc;
}
int tg_copy_obs_feature(tg_ctx* c, float* dst, int32_t terminal) { return copy_entry(c, TG_OBS_KEY_FEATURE, terminal, kPlain, "tg_copy_obs_feature", dst); }
int tg_get_obs_oracle(tg_ctx* c, void** p, int32_t* dim) {
    const int rc = get_entry(c, TG_OBS_KEY_ORACLE, 0, kPlain, "tg_get_obs_oracle", p);
    if (rc == 0 && dim) *dim = oracle_dim(c);
    return rc;
}
int tg_copy_obs_oracle(tg_ctx* c, float* dst) { return copy_entry(c, TG_OBS_KEY_ORACLE, 0, kPlain, "tg_copy_obs_oracle", dst); }
int tg_get_obs_oracle_terminal(tg_ctx* c, void** p) { return get_entry(c, TG_OBS_KEY_ORACLE, 1, kPlain, "tg_get_obs_oracle_terminal", p); }
int tg_copy_obs_oracle_terminal(tg_ctx* c, float* dst) { return copy_entry(c, TG_OBS_KEY_ORACLE, 1, kPlain, "tg_copy_obs_oracle_terminal", dst); }
int tg_copy_obs_rows(tg_ctx* c, int32_t visual, int32_t terminal, const int32_t* env_ids, int32_t count, uint8_t* dst) {
    return rows_entry(c, visual ? TG_OBS_KEY_VISUAL : TG_OBS_KEY_TACTILE, terminal, kPlain, "tg_copy_obs_rows", env_ids, count, dst);
}
int tg_get_obs_stack(tg_ctx* c, int32_t key, int32_t terminal, void** p) { return get_entry(c, key, terminal, kStacked, "tg_get_obs_stack", p); }
int tg_copy_obs_stack(tg_ctx* c, int32_t key, int32_t terminal, void* dst) { return copy_entry(c, key, terminal, kStacked, "tg_copy_obs_stack", dst); }
int tg_copy_obs_stack_rows(tg_ctx* c, int32_t key, int32_t terminal, const int32_t* env_ids, int32_t count, void* dst) {
    return rows_entry(c, key, terminal, kStacked, "tg_copy_obs_stack_rows", env_ids, count, dst);
}

int tg_get_reward_done_dev(tg_ctx* c, void** r, void** d) {
    if (!c) return fail(-1, "NULL ctx");
    if (r) *r = c->st.reward;
    if (d) *d = c->st.done;
    return 0;
}
int tg_get_reward_done(tg_ctx* c, float* reward, uint8_t* done) {
    if (!c) return fail(-1, "NULL ctx");
    TG_ENTER(c);
    const int n = c->cfg.num_envs;
    if (reward) TG_HIP(hipMemcpyAsync(reward, c->st.reward, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (done) TG_HIP(hipMemcpyAsync(done, c->st.done, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int tg_get_packed_outputs(tg_ctx* c, void** p, int64_t* obs_bytes, int64_t* total_bytes) {
    if (!c || !p) return fail(-1, "NULL argument");
    *p = c->d_obs;
    if (obs_bytes) *obs_bytes = (int64_t)c->packed_obs_bytes;
    if (total_bytes) *total_bytes = (int64_t)c->packed_bytes;
    return 0;
}
int tg_get_packed_feature(tg_ctx* c, int64_t* feature_off, int32_t* dim) {
    if (!c || !feature_off) return fail(-1, "NULL argument");
    const bool has = env_has_feature(c->cfg.env_kind);
    *feature_off = has ? (int64_t)c->packed_feature_off : -1;
    if (dim) *dim = has ? 12 : 0;
    return 0;
}

int tg_set_frame_stack(tg_ctx* c, int32_t n) {
    if (!c) return fail(-1, "NULL ctx");
    if (n < 1 || n > kStackMax) return fail(-1, "tg_set_frame_stack: n must be in [1, 8]");
    if (n > 1 && (c->obs_ext[0] || c->obs_ext[1])) return fail(-1, "tg_set_frame_stack: not with render targets of the caller (tg_set_obs_targets: sharded runs)");
    TG_ENTER(c);
    return alloc_stacks(c, n, c->obs_cf);
}
int tg_set_obs_layout(tg_ctx* c, int32_t channels_first) {
    if (!c) return fail(-1, "NULL ctx");
    if (channels_first != 0 && channels_first != 1) return fail(-1, "tg_set_obs_layout: channels_first must be 0 or 1");
    if (channels_first && (c->obs_ext[0] || c->obs_ext[1])) return fail(-1, "tg_set_obs_layout: not with render targets of the caller (tg_set_obs_targets: sharded runs)");
    TG_ENTER(c);
    return alloc_stacks(c, c->stack_n, channels_first);
}
int tg_get_obs_layout(tg_ctx* c, int32_t* channels_first) {
    if (!c || !channels_first) return fail(-1, "NULL argument");
    *channels_first = c->obs_cf;
    return 0;
}
int tg_get_frame_stack(tg_ctx* c, int32_t* n) {
    if (!c || !n) return fail(-1, "NULL argument");
    *n = c->stack_n;
    return 0;
}

}  // extern "C"
