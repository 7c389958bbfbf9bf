// Rank of a lane among the lanes of its half-wave that fall in the same class, from wave ballots.
//
// The row rotation (bsk_rowrot.hpp, bsk_uniform.hpp) gives every lane its rank among the active lanes of its
// half-wave whose window base lies in the same class; only the rank mod the order is used.  One ballot per bit of
// the class puts the whole wave's classes into scalar registers; a lane XNORs each ballot with its own bit
// (replicated over the word) and ANDs the results together with the active lanes of its half below it: those are
// its class mates in lower lanes, and the rank is their number.  No LDS traffic.
//
// rank_from_ballots holds everything after the ballots and compiles for the host (tests/rank_mask_check.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BSK_RANK_HD __host__ __device__
#else
#define BSK_RANK_HD
#endif

namespace bsk {

// Each step `mates & ~(ballot ^ bit)` is one three-input bit operation on gfx950 when it is selected on its own.
#if defined(__HIP_DEVICE_COMPILE__)
#define BSK_RANK_STEP(x) asm volatile("" : "+v"(x))
#else
#define BSK_RANK_STEP(x) (void)0
#endif

// b[k]: the ballot of class bit k over the wave (inactive lanes contribute 0); active: the ballot of the active
// lanes; cls: the lane's class, < 2^NB.  Ranks inside a class and a half-wave are 0, 1, 2, ... in lane order.
// Both halves' words are carried to the end: choosing a lane's half word of every ballot costs more than the
// second word's three operations, and the half is chosen once, by the mask of the lanes below.
template <int NB>
BSK_RANK_HD inline int rank_from_ballots(const unsigned long long (&b)[NB], unsigned long long active, unsigned cls, int lane)
{
    // the active lanes of this lane's half-wave below it
    const unsigned lt = (1u << (lane & 31)) - 1u;
    unsigned lo = (unsigned)active & ((lane & 32) ? 0u : lt);
    unsigned hi = (unsigned)(active >> 32) & ((lane & 32) ? lt : 0u);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const unsigned bit = 0u - ((cls >> k) & 1u);              // the lane's bit k on all 32 positions
        lo &= ~((unsigned)b[k] ^ bit);
        BSK_RANK_STEP(lo);
        hi &= ~((unsigned)(b[k] >> 32) ^ bit);
        BSK_RANK_STEP(hi);
    }
    return __builtin_popcount(lo) + __builtin_popcount(hi);
}

#if defined(__HIPCC__)
// The ballots themselves: one v_cmp into a scalar pair per class bit, executed by the active lanes only.
template <int NB>
__device__ __forceinline__ int ballot_rank(unsigned cls, int lane)
{
    const unsigned long long act = __ballot(1);
    unsigned long long b[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) b[k] = __ballot((cls >> k) & 1u);
    return rank_from_ballots<NB>(b, act, cls, lane);
}
#endif

}  // namespace bsk
