// tg_stack.hip - the device frame stack (tg_set_frame_stack): stable_baselines3's VecFrameStack over the observation buffers, one launch per step /
// reset on the context's stream, after the observations of that step / reset are complete.
//
// Images: one workgroup per (env, 16 blocks of 16 x 16 pixels); a lane per block row, 16-byte frame accesses and 16 * n-byte stack accesses.  A block
// is read and written only if the new frame's block differs from the template image or one of its slots does not hold the template (the per-block
// record, one bit per slot): otherwise every slot holds the template before and after the shift, and there is nothing to move.  That holds whatever
// drew the frame.  A zeroed slot counts as "not the template", so after a done or a reset the block is rewritten until the zeros have left.
// TG_STACK_REWRITE_ALL=1 (tests) processes every block.
// Vectors: a second phase of the same launch, a lane per (env, element), looping over the slots.
// A finished env's terminal stack is assembled from the old stack by the lane that then overwrites that stack: there is no order to keep between lanes.
//
// k_obs_stack (tg_set_obs_layout, visual keys): the same rules in the layouts k_frame_stack does not write.
//   Tactile, channels first [N][n][H][W]: the shift moves whole planes (slot s <- slot s + 1), 16 bytes per lane and slot, no byte shuffle; the same
//   workgroups, per-block template record and unchanged-block skip as k_frame_stack.
//   Visual [N][H][W][3] frames (no template: every lane works): a lane per 16 pixels of a row.  Channels last [N][H][W][3n]: 48 n bytes per lane
//   (3 n dwordx4), shifted by 3 bytes per slot in registers.  Channels first [N][3n][H][W]: the frame's 48 bytes de-interleaved into three 16-byte
//   colour planes, older slots moved plane by plane.
//   Vectors (channels first): k_frame_stack's vector phase (stack_vec_lane), so that one launch writes every key.
#include "tg_stack.h"

namespace tg {

// Byte k of a little-endian word array (k is a compile-time constant once the loops below are unrolled: the arrays stay in registers).
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// One block row of NS slots: 16 pixels x NS bytes.  out = the row after the shift: slot s takes old slot s + 1 (ZERO: 0), the newest slot takes the frame.
template <int NS, bool ZERO>
__device__ __forceinline__ void shift_row(const uint32_t (&old)[4 * NS], const uint32_t (&fr)[4], uint32_t (&out)[4 * NS]) {
#pragma unroll
    for (int q = 0; q < 4 * NS; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * q + b, p = k / NS, s = k % NS;
            const uint32_t x = s == NS - 1 ? byte_of(fr, p) : (ZERO ? 0u : byte_of(old, k + 1));
            v |= x << (8 * b);
        }
        out[q] = v;
    }
}

template <int NS>
__device__ __forceinline__ void load_row(const uint8_t* p, uint32_t (&w)[4 * NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint4 u = reinterpret_cast<const uint4*>(p)[i];
        w[4 * i] = u.x; w[4 * i + 1] = u.y; w[4 * i + 2] = u.z; w[4 * i + 3] = u.w;
    }
}
template <int NS>
__device__ __forceinline__ void store_row(uint8_t* p, const uint32_t (&w)[4 * NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) reinterpret_cast<uint4*>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

template <int NS>
__global__ __launch_bounds__(256) void k_frame_stack(StackArgs a, int img_groups) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < img_groups) {
        const int bpr = a.W >> 4, nb = (a.H >> 4) * bpr, gpe = nb >> 4;   // blocks per block row, per env; workgroups per env
        const int e = blockIdx.x / gpe;
        const bool f = a.flag ? a.flag[e] != 0 : true;
        if (a.mode == kStackReset && !f) return;                           // (uniform over the workgroup: one env)
        const int b = (blockIdx.x - e * gpe) * 16 + (tid >> 4);
        const int y = (b / bpr) * 16 + (tid & 15), x0 = (b % bpr) * 16;
        const size_t pix = ((size_t)e * a.H + y) * a.W + x0;
        const uint4 f4 = *reinterpret_cast<const uint4*>(a.frame + pix);
        const uint4 t4 = *reinterpret_cast<const uint4*>(a.tmpl + (size_t)y * a.W + x0);
        const bool neq = f4.x != t4.x || f4.y != t4.y || f4.z != t4.z || f4.w != t4.w;
        const bool blk_neq = ((__ballot(neq) >> (tid & 48)) & 0xffffull) != 0ull;   // any row of this block (16 lanes of the wavefront)
        uint8_t* rp = a.rec + (size_t)e * nb + b;
        const uint32_t rec = *rp, full = (1u << NS) - 1u, eq_bit = blk_neq ? 0u : (1u << (NS - 1));
        if (!f && !a.rewrite_all && !blk_neq && rec == full) return;     // every slot and the new frame are the template here
        const uint32_t fr[4] = {f4.x, f4.y, f4.z, f4.w};
        uint8_t* sp = a.stack + pix * NS;
        uint32_t out[4 * NS];
        if (!f) {
            uint32_t old[4 * NS];
            load_row<NS>(sp, old);
            shift_row<NS, false>(old, fr, out);
        } else {
            if (a.mode == kStackStep && a.term_stack) {                    // terminal stack: the old stack's newest n - 1 slots, then the terminal frame
                uint32_t old[4 * NS], tout[4 * NS];
                load_row<NS>(sp, old);
                const uint4 g4 = *reinterpret_cast<const uint4*>(a.term_frame + pix);
                const uint32_t tf[4] = {g4.x, g4.y, g4.z, g4.w};
                shift_row<NS, false>(old, tf, tout);
                store_row<NS>(a.term_stack + pix * NS, tout);
            }
            shift_row<NS, true>(out, fr, out);                            // (ZERO: `old` is not read)
        }
        store_row<NS>(sp, out);
        if ((tid & 15) == 0) *rp = (uint8_t)((f ? 0u : (rec >> 1)) | eq_bit);
        return;
    }
    // vectors: lane t of this phase -> (key, env, element)
    int idx = ((int)blockIdx.x - img_groups) * 256 + tid;
    const int n0 = a.num_envs * a.vec[0].dim;
    const bool k1 = idx >= n0;
    if (k1) idx -= n0;
    const StackVec v = k1 ? a.vec[1] : a.vec[0];
    if (idx >= a.num_envs * v.dim) return;
    const int e = idx / v.dim, j = idx - e * v.dim;
    const bool f = a.flag ? a.flag[e] != 0 : true;
    if (a.mode == kStackReset && !f) return;
    uint32_t* row = reinterpret_cast<uint32_t*>(v.stack) + (size_t)e * v.dim * NS + j;   // slot s at row[s * dim]: bits are moved, not values
    const uint32_t src = reinterpret_cast<const uint32_t*>(v.src)[(size_t)e * v.pitch + j];
    uint32_t old[NS];
    if (!f || (a.mode == kStackStep && v.term_stack)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) old[s] = row[s * v.dim];
    }
    if (f && a.mode == kStackStep && v.term_stack) {
        uint32_t* trow = reinterpret_cast<uint32_t*>(v.term_stack) + (size_t)e * v.dim * NS + j;
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) trow[s * v.dim] = old[s + 1];
        trow[(NS - 1) * v.dim] = reinterpret_cast<const uint32_t*>(v.term)[(size_t)e * v.pitch + j];
    }
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) row[s * v.dim] = f ? 0u : old[s + 1];
    row[(NS - 1) * v.dim] = src;
}

int launch_frame_stack(const StackArgs& a, hipStream_t stream) {
    if (a.n < 2 || a.n > kStackMax || a.num_envs <= 0) return -1;
    long img = 0;
    if (a.frame) {
        const int nb = (a.H / 16) * (a.W / 16);
        if (a.H % 16 || a.W % 16 || nb % 16 || !a.tmpl || !a.stack || !a.rec) return -1;
        img = (long)a.num_envs * (nb / 16);
    }
    for (const StackVec& v : a.vec)
        if (v.dim < 0 || (v.dim > 0 && (!v.src || !v.stack || v.pitch < v.dim))) return -1;
    const long groups = img + ((long)a.num_envs * (a.vec[0].dim + a.vec[1].dim) + 255) / 256;
    if (groups == 0) return 0;
    if (groups > 0x7fffffffL) return -1;
    const dim3 grid((unsigned)groups), block(256);
    switch (a.n) {
        case 2: hipLaunchKernelGGL(k_frame_stack<2>, grid, block, 0, stream, a, (int)img); break;
        case 3: hipLaunchKernelGGL(k_frame_stack<3>, grid, block, 0, stream, a, (int)img); break;
        case 4: hipLaunchKernelGGL(k_frame_stack<4>, grid, block, 0, stream, a, (int)img); break;
        case 5: hipLaunchKernelGGL(k_frame_stack<5>, grid, block, 0, stream, a, (int)img); break;
        case 6: hipLaunchKernelGGL(k_frame_stack<6>, grid, block, 0, stream, a, (int)img); break;
        case 7: hipLaunchKernelGGL(k_frame_stack<7>, grid, block, 0, stream, a, (int)img); break;
        default: hipLaunchKernelGGL(k_frame_stack<8>, grid, block, 0, stream, a, (int)img); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- k_obs_stack ----

// The vector phase of k_frame_stack as a function (k_frame_stack keeps its own text: its code is unchanged by this kernel's addition).
template <int NS>
__device__ __forceinline__ void stack_vec_lane(const StackArgs& a, int idx) {
    const int n0 = a.num_envs * a.vec[0].dim;
    const bool k1 = idx >= n0;
    if (k1) idx -= n0;
    const StackVec v = k1 ? a.vec[1] : a.vec[0];
    if (idx >= a.num_envs * v.dim) return;
    const int e = idx / v.dim, j = idx - e * v.dim;
    const bool f = a.flag ? a.flag[e] != 0 : true;
    if (a.mode == kStackReset && !f) return;
    uint32_t* row = reinterpret_cast<uint32_t*>(v.stack) + (size_t)e * v.dim * NS + j;
    const uint32_t src = reinterpret_cast<const uint32_t*>(v.src)[(size_t)e * v.pitch + j];
    uint32_t old[NS];
    if (!f || (a.mode == kStackStep && v.term_stack)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) old[s] = row[s * v.dim];
    }
    if (f && a.mode == kStackStep && v.term_stack) {
        uint32_t* trow = reinterpret_cast<uint32_t*>(v.term_stack) + (size_t)e * v.dim * NS + j;
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) trow[s * v.dim] = old[s + 1];
        trow[(NS - 1) * v.dim] = reinterpret_cast<const uint32_t*>(v.term)[(size_t)e * v.pitch + j];
    }
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) row[s * v.dim] = f ? 0u : old[s + 1];
    row[(NS - 1) * v.dim] = src;
}

__device__ __forceinline__ uint4 ld16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st16(uint8_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

// Tactile, channels first: one block row (16 bytes) of every plane of env e's stack per lane; g = the workgroup's index among the image workgroups.
template <int NS>
__device__ __forceinline__ void stack_planar_rows(const StackArgs& a, int g, int tid) {
    const int bpr = a.W >> 4, nb = (a.H >> 4) * bpr, gpe = nb >> 4;
    const int e = g / gpe;
    const bool f = a.flag ? a.flag[e] != 0 : true;
    if (a.mode == kStackReset && !f) return;
    const int b = (g - e * gpe) * 16 + (tid >> 4);
    const int y = (b / bpr) * 16 + (tid & 15), x0 = (b % bpr) * 16;
    const size_t plane = (size_t)a.H * a.W, off = (size_t)y * a.W + x0;
    const uint4 f4 = ld16(a.frame + e * plane + off);
    const uint4 t4 = ld16(a.tmpl + off);
    const bool neq = f4.x != t4.x || f4.y != t4.y || f4.z != t4.z || f4.w != t4.w;
    const bool blk_neq = ((__ballot(neq) >> (tid & 48)) & 0xffffull) != 0ull;
    uint8_t* rp = a.rec + (size_t)e * nb + b;
    const uint32_t rec = *rp, full = (1u << NS) - 1u, eq_bit = blk_neq ? 0u : (1u << (NS - 1));
    if (!f && !a.rewrite_all && !blk_neq && rec == full) return;
    uint8_t* sp = a.stack + (size_t)e * NS * plane + off;             // slot s at sp + s * plane
    uint4 old[NS];                                                    // old[s] = slot s + 1 (s < NS - 1): every load before any store
    if (!f || (a.mode == kStackStep && a.term_stack)) {
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) old[s] = ld16(sp + (s + 1) * plane);
    }
    if (f) {
        if (a.mode == kStackStep && a.term_stack) {
            uint8_t* tp = a.term_stack + (size_t)e * NS * plane + off;
#pragma unroll
            for (int s = 0; s < NS - 1; ++s) st16(tp + s * plane, old[s]);
            st16(tp + (NS - 1) * plane, ld16(a.term_frame + e * plane + off));
        }
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) st16(sp + s * plane, make_uint4(0u, 0u, 0u, 0u));
    } else {
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) st16(sp + s * plane, old[s]);
    }
    st16(sp + (NS - 1) * plane, f4);
    if ((tid & 15) == 0) *rp = (uint8_t)((f ? 0u : (rec >> 1)) | eq_bit);
}

// Visual, channels last: 16 pixels x NS slots x 3 bytes.  out = the row after the shift: slot s takes old slot s + 1 (ZERO: 0), the newest slot
// takes the frame's pixel.  out may be old: word q is written after every word it reads (q and q + 1).
template <int NS, bool ZERO>
__device__ __forceinline__ void shift_row_rgb(const uint32_t (&old)[12 * NS], const uint32_t (&fr)[12], uint32_t (&out)[12 * NS]) {
#pragma unroll
    for (int q = 0; q < 12 * NS; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * q + b, p = k / (3 * NS), r = k % (3 * NS);
            const uint32_t x = r >= 3 * (NS - 1) ? byte_of(fr, 3 * p + r - 3 * (NS - 1)) : (ZERO ? 0u : byte_of(old, k + 3));
            v |= x << (8 * b);
        }
        out[q] = v;
    }
}

// Colour plane c of 16 interleaved rgb pixels (48 bytes).
__device__ __forceinline__ uint4 rgb_plane(const uint32_t (&fr)[12], int c) {
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= byte_of(fr, 3 * (4 * q + b) + c) << (8 * b);
        w[q] = v;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Visual: lane = global index of a 16-pixel run of one image row (env e = lane / runs per image).
template <int NS, bool CF>
__device__ __forceinline__ void stack_visual_run(const StackArgs& a, const VisStack& v, int lane) {
    const int rpe = (v.H * v.W) >> 4;
    if (lane >= a.num_envs * rpe) return;
    const int e = lane / rpe;
    const bool f = a.flag ? a.flag[e] != 0 : true;
    if (a.mode == kStackReset && !f) return;
    const bool term = f && a.mode == kStackStep && v.term_stack;
    uint32_t fr[12];
    load_row<3>(v.frame + (size_t)lane * 48, fr);
    if (!CF) {
        uint8_t* sp = v.stack + (size_t)lane * 48 * NS;
        uint32_t w[12 * NS];
        if (!f || term) load_row<3 * NS>(sp, w);
        if (term) {
            uint32_t tf[12];
            load_row<3>(v.term_frame + (size_t)lane * 48, tf);
            shift_row_rgb<NS, false>(w, tf, w);
            store_row<3 * NS>(v.term_stack + (size_t)lane * 48 * NS, w);
        }
        if (f) shift_row_rgb<NS, true>(w, fr, w);
        else shift_row_rgb<NS, false>(w, fr, w);
        store_row<3 * NS>(sp, w);
    } else {
        const size_t plane = (size_t)v.H * v.W, off = (size_t)(lane - e * rpe) * 16;
        uint8_t* sp = v.stack + (size_t)e * 3 * NS * plane + off;       // colour c of slot s at sp + (3 s + c) * plane
        uint4 old[3 * NS];                                               // old[i] = plane i + 3 (i < 3 (NS - 1))
        if (!f || term) {
#pragma unroll
            for (int i = 0; i < 3 * (NS - 1); ++i) old[i] = ld16(sp + (i + 3) * plane);
        }
        if (term) {
            uint8_t* tp = v.term_stack + (size_t)e * 3 * NS * plane + off;
            uint32_t tf[12];
            load_row<3>(v.term_frame + (size_t)lane * 48, tf);
#pragma unroll
            for (int i = 0; i < 3 * (NS - 1); ++i) st16(tp + i * plane, old[i]);
#pragma unroll
            for (int c = 0; c < 3; ++c) st16(tp + (3 * (NS - 1) + c) * plane, rgb_plane(tf, c));
        }
#pragma unroll
        for (int i = 0; i < 3 * (NS - 1); ++i) st16(sp + i * plane, f ? make_uint4(0u, 0u, 0u, 0u) : old[i]);
#pragma unroll
        for (int c = 0; c < 3; ++c) st16(sp + (3 * (NS - 1) + c) * plane, rgb_plane(fr, c));
    }
}

// Workgroups: [img_groups: tactile, channels first] [vis_groups: visual] [the rest: vectors, channels first].
template <int NS, bool CF>
__global__ __launch_bounds__(256) void k_obs_stack(StackArgs a, VisStack v, int img_groups, int vis_groups) {
    const int tid = threadIdx.x, g = (int)blockIdx.x;
    if (g < img_groups) {
        if (CF && NS > 1) stack_planar_rows<NS>(a, g, tid);
        return;
    }
    if (g < img_groups + vis_groups) {
        stack_visual_run<NS, CF>(a, v, (g - img_groups) * 256 + tid);
        return;
    }
    if (CF && NS > 1) stack_vec_lane<NS>(a, (g - img_groups - vis_groups) * 256 + tid);
}

template <int NS>
static void launch_obs_n(bool cf, dim3 grid, const StackArgs& o, const VisStack& v, int img, int vis, hipStream_t stream) {
    if (cf) hipLaunchKernelGGL((k_obs_stack<NS, true>), grid, dim3(256), 0, stream, o, v, img, vis);
    else hipLaunchKernelGGL((k_obs_stack<NS, false>), grid, dim3(256), 0, stream, o, v, img, vis);
}

int launch_obs_stack(const StackArgs& a, const VisStack& v, int channels_first, hipStream_t stream) {
    if (a.n < 1 || a.n > kStackMax || a.num_envs <= 0) return -1;
    // (the visual key is checked before k_frame_stack is launched: a refused call writes nothing)
    if (v.frame && (v.H <= 0 || v.W <= 0 || v.W % 16 || !v.stack || (!channels_first && a.n < 2))) return -1;
    StackArgs o = a;                                   // what k_obs_stack writes besides the visual image
    if (!channels_first) {
        if (a.n >= 2) {
            if (int rc = launch_frame_stack(a, stream)) return rc;
        }
        o.frame = nullptr;
        o.vec[0].dim = o.vec[1].dim = 0;
    }
    long img = 0, vis = 0;
    if (o.frame) {
        const int nb = (o.H / 16) * (o.W / 16);
        if (o.n < 2 || o.H % 16 || o.W % 16 || nb % 16 || !o.tmpl || !o.stack || !o.rec) return -1;
        img = (long)o.num_envs * (nb / 16);
    }
    if (v.frame) vis = ((long)o.num_envs * (v.H * v.W / 16) + 255) / 256;
    for (const StackVec& x : o.vec)
        if (x.dim < 0 || (x.dim > 0 && (o.n < 2 || !x.src || !x.stack || x.pitch < x.dim))) return -1;
    const long groups = img + vis + ((long)o.num_envs * (o.vec[0].dim + o.vec[1].dim) + 255) / 256;
    if (groups == 0) return 0;
    if (groups > 0x7fffffffL) return -1;
    const dim3 grid((unsigned)groups);
    const bool cf = channels_first != 0;
    switch (a.n) {
        case 1: launch_obs_n<1>(true, grid, o, v, (int)img, (int)vis, stream); break;   // (channels last with n = 1 has no stack: tg_set_obs_layout)
        case 2: launch_obs_n<2>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        case 3: launch_obs_n<3>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        case 4: launch_obs_n<4>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        case 5: launch_obs_n<5>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        case 6: launch_obs_n<6>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        case 7: launch_obs_n<7>(cf, grid, o, v, (int)img, (int)vis, stream); break;
        default: launch_obs_n<8>(cf, grid, o, v, (int)img, (int)vis, stream); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace tg
