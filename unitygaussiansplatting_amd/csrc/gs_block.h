// gs_block.h -- the device building blocks the edit path's kernels share (gs_edit / gs_attributes / gs_neighbours / gs_export / gs_bake / gs_compact .hip):
// wave reductions, bit buffers, the alive test, the selection write, and the two pieces of a compaction -- the rank of a lane inside its 256-thread
// workgroup and the workgroup's min / max of a position.  Header-only and wave64; every helper that names a workgroup means 256 threads = four waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_device_math.h"

namespace gs {

// over the 64 lanes, every lane gets the result: the xor butterfly 32 .. 1
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// the word of a 64-bit ballot this lane's splat belongs to
__device__ __forceinline__ uint32_t ballot_word(unsigned long long b, uint32_t lane) { return (uint32_t)(b >> (lane & 32u)); }

// bit idx of a 1-bit-per-splat buffer
__device__ __forceinline__ bool bit_set(const uint32_t* words, uint32_t idx) { return ((words[idx >> 5] >> (idx & 31u)) & 1u) != 0u; }

// alive = idx < N, not deleted, not cut (ExportPlyFile's rule; the test of every edit kernel); also hands back the position and the cut flag
__device__ __forceinline__ bool export_alive(const gsm::AssetView& a, const gsm::EditView& e, uint32_t idx, uint32_t ci, gsm::V3& pos, bool& cut) {
    cut = false;
    pos = { 0.0f, 0.0f, 0.0f };
    if (idx >= a.n) return false;
    pos = gsm::LoadSplatPosChunk(a, idx, ci);
    cut = gsm::IsSplatCut(e, pos.x, pos.y, pos.z);
    const bool deleted = e.deletedBits && bit_set(e.deletedBits, idx);
    return !cut && !deleted;
}

// selected |= pred (subtract: &= ~pred) for the splat idx of every lane, one thread per splat in index order: the predicate becomes a word through
// __ballot, a wave owns two consecutive words, lanes 0 and 32 do a plain read-modify-write of theirs -- no other wave touches that word -- and
// nothing is stored at or beyond nWords.  Every lane of the wave calls it
__device__ __forceinline__ void selection_apply(bool pred, uint32_t idx, uint32_t lane, uint32_t* sel, uint32_t nWords, uint32_t subtract) {
    const uint32_t word = ballot_word(__ballot(pred), lane);
    const uint32_t w = idx >> 5;
    if ((lane & 31u) == 0u && w < nWords && word) sel[w] = subtract ? (sel[w] & ~word) : (sel[w] | word);
}

// The rank of a lane among the lanes of its workgroup that hold `mine`, in two steps around the caller's __syncthreads().  Before it, block_rank:
// the rank inside the wave, and s_cnt[wave] = the wave's count.  After it, block_first: `first` + the counts of the waves before this one
__device__ __forceinline__ uint32_t block_rank(bool mine, uint32_t lane, uint32_t wave, uint32_t s_cnt[4]) {
    const unsigned long long bal = __ballot(mine);
    if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(bal);
    return (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ uint32_t block_first(const uint32_t s_cnt[4], uint32_t wave, uint32_t first) {
    for (uint32_t w = 0; w < wave; ++w) first += s_cnt[w];
    return first;
}

// partial[0..2 / 3..5] = min / max of p over the lanes of the workgroup that hold `mine` (+inf / -inf: none), the same two steps.  Before the
// barrier, block_bounds: the butterfly inside each wave into s_red[wave].  After it, block_bounds_store: threads 0 .. 5 fold the four waves as
// f(f(0, 1), f(2, 3)) and store one float each.  MAX = false: the minima alone, three partials (the neighbour grid wants nothing but its origin, and
// the second butterfly costs its list kernel a fifth of the stage)
template <bool MAX = true>
__device__ __forceinline__ void block_bounds(bool mine, const float p[3], uint32_t lane, uint32_t wave, float s_red[4][6]) {
    const float inf = gsm::u2f(0x7f800000u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mn = wave_min(mine ? p[c] : inf);
        if (lane == 0u) s_red[wave][c] = mn;
        if (MAX) {
            const float mx = wave_max(mine ? p[c] : -inf);
            if (lane == 0u) s_red[wave][3 + c] = mx;
        }
    }
}
template <bool MAX = true>
__device__ __forceinline__ void block_bounds_store(const float s_red[4][6], float* __restrict__ partial) {
    const uint32_t t = threadIdx.x;
    if (t < 3u) partial[t] = fminf(fminf(s_red[0][t], s_red[1][t]), fminf(s_red[2][t], s_red[3][t]));
    else if (MAX && t < 6u) partial[t] = fmaxf(fmaxf(s_red[0][t], s_red[1][t]), fmaxf(s_red[2][t], s_red[3][t]));
}

} // namespace gs
