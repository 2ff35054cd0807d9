// tg_copy_units.hpp - what the table-driven copy kernels share (tg_rollout.hip: k_rollout_add, k_rollout_gather; tg_replay.hip: k_replay_add).
//
// A copy kernel moves `units` of 16, 4 or 1 bytes: the widest that divides an array's byte count (per row where rows are addressed) and every one
// of its addresses, chosen on the host per array.  A lane moves up to four units 256 apart (loads first, then stores), a workgroup 1024
// consecutive units of ONE array; the workgroup -> array map is a prefix table of workgroup counts passed by value with the pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"

namespace tg {

constexpr int kRoMax = TG_ROLLOUT_MAX_ARRAYS;
constexpr int kRoThreads = 256;
constexpr int kRoPerBlock = 1024;   // units per workgroup: 4 per lane

struct RoTable {
    const uint8_t* src[kRoMax];
    uint8_t* dst[kRoMax];
    int64_t units[kRoMax];      // add: units of the array; gather: units of one row
    int32_t unit[kRoMax];       // 16, 4 or 1 bytes; add, flag arrays: 0 (one uint8 flag in, one float32 0 / 1 out)
    uint32_t blk_end[kRoMax];   // workgroups of arrays 0 .. i
    int32_t n;
};

template <typename V>
__device__ __forceinline__ void move4(const uint8_t* const (&s)[4], uint8_t* const (&d)[4], const bool (&on)[4]) {
    V v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (on[k]) v[k] = *reinterpret_cast<const V*>(s[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (on[k]) *reinterpret_cast<V*>(d[k]) = v[k];
}

// V16, the 16-byte register type: with HIP's uint4 (a struct) the compiler keeps move4's four values in a 16 KiB LDS array per workgroup, which is
// what k_rollout_add and k_rollout_gather are built and measured with; with the native vector u32x4 they stay in registers (k_replay_add).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename V16 = uint4>
__device__ __forceinline__ void move_units(int unit, const uint8_t* const (&s)[4], uint8_t* const (&d)[4], const bool (&on)[4]) {
    if (unit == 16) move4<V16>(s, d, on);           // `unit` is the same in every lane of the workgroup
    else if (unit == 4) move4<uint32_t>(s, d, on);
    else move4<uint8_t>(s, d, on);
}

// The array of this workgroup and its first unit there (any table with `n` and `blk_end`).
template <typename Table>
__device__ __forceinline__ int which_array(const Table& t, int64_t& u0) {
    int a = 0;
    uint32_t first = 0;
#pragma unroll
    for (int i = 0; i < kRoMax - 1; ++i)
        if (i < t.n - 1 && blockIdx.x >= t.blk_end[i]) { a = i + 1; first = t.blk_end[i]; }
    u0 = (int64_t)(blockIdx.x - first) * kRoPerBlock;
    return a;
}

// Table fields are read with a uniform index through selects over the by-value table (no indexed private array: no scratch).
#define RO_PICK(field, a, out)                    \
    do {                                          \
        out = t.field[0];                         \
        _Pragma("unroll") for (int i = 1; i < kRoMax; ++i) if (i == (a)) out = t.field[i]; \
    } while (0)

static inline int widest_unit(uintptr_t a, uintptr_t b, int64_t bytes) {
    const uintptr_t m = a | b | (uintptr_t)bytes;
    return !(m & 15) ? 16 : !(m & 3) ? 4 : 1;
}

// Appends the workgroups of an array of `total` units; false when the grid would pass 2^31 workgroups.
template <typename Table>
static inline bool push_blocks(Table& t, int i, int64_t total) {
    const int64_t blocks = (total + kRoPerBlock - 1) / kRoPerBlock;
    const int64_t end = (i ? (int64_t)t.blk_end[i - 1] : 0) + blocks;
    if (end >= ((int64_t)1 << 31)) return false;
    t.blk_end[i] = (uint32_t)end;
    return true;
}

}  // namespace tg
