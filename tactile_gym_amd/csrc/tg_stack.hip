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

}  // namespace tg
