// gs_edit.hip -- selection and deletion: the edit kernels of SplatUtilities.compute that never write the asset, and the
// gs_renderer_edit_* entry points over them (GaussianSplatRenderer.Edit*, GaussianSplatRenderer.cs:705-740,767-840,896-934).
//
// Restated word for word in what they leave in memory:
//   CSInitEditData + CSUpdateEditData  SplatUtilities.compute:266-325   counts of selected / deleted / cut splats, bounds of the selection
//   CSClearBuffer                      :327-334                         (a memset)
//   CSInvertSelection / CSSelectAll    :336-377                         every bit, cut splats cleared
//   CSOrBuffers                        :380-389                         deleted |= selected
//   CSSelectionUpdate                  :391-423                         rectangle selection through a camera, add or subtract
//   CSTranslateSelection / CSRotateSelection / CSScaleSelection  :425-521  the selected splats' positions (and rotation words) rewritten
// The last three are the only kernels that write splat data.  The asset's blobs are shared between contexts, lanes and replicas and stay
// immutable: the first transform whose format gate can pass gives the renderer a private copy of the pos and / or other blob (copy-on-write,
// gs::asset_view), and from then on every kernel of this renderer and of its lanes reads that copy.  With gs_renderer_edit_set_rigid_transforms on,
// rotate and uniform scale also do what the reference's three @TODOs leave out -- orientation on the right side, SH rotated, splat sizes scaled -- and
// the SH blob becomes private the same way (the RIGID instantiations below).  Undo and redo of all of this, which the
// reference does not have, is the edit history: a journal of the bit buffers and of the selected splats' records (hist_*).
// CSExportData only reads: gs_export.hip.
// CSCopySplats / EditSetSplatCount / EditCopySplatsInto -- the merge -- are gs_copy.hip.  The highlight of selected splats
// (RenderGaussianSplats.shader:63-73,87-101) is drawn by calc_view and the blend (gs_view.hip, gs_raster.hip) when
// gs_renderer_set_selection_highlight is on; what this file does for it is keep the lanes' copies of the selection in step
// (edit_selected_to_lanes).  With the switch off -- the default -- selection has no visual effect.
//
// Shape (wave64; not the reference's, which runs one thread per WORD with a 32-iteration position loop, neighbouring threads reading
// positions 32 records apart): one thread per SPLAT, 256-thread workgroups aligned to the 256-splat chunk so that the chunk header is
// workgroup-uniform.  The per-splat predicate (cut / hit) becomes a word through __ballot (ballot_word, gs_block.h, which also holds the
// read-modify-write the later selection tools share, selection_apply); a wave owns exactly two consecutive words, one
// lane per word does a plain read-modify-write -- no other wave touches that word, so the reference's per-splat InterlockedOr / And is not
// needed and the result is identical.  No word index >= ceil(N/32) is ever stored.  Counts are popcounts of the words, bounds reduce per
// wave with __shfl_xor and across the four waves in LDS: at most nine global atomics per workgroup.
//
// Two literal quirks of the reference, kept:
//   - CSSelectAll / CSInvertSelection set the bits of the last word beyond N, and CSUpdateEditData counts them: N = 33, select all ->
//     selected = 64.  The words and the counts are the parity surface, so they are the reference's.
//   - a splat whose pixel position is NaN is inside every rectangle (all four comparisons are false).
// One difference: the bounds are reduced as sortable uints at every level (a total order, so any grouping gives the same bits); a
// component that is +0 for one selected splat and -0 for another reports -0, where the reference leaves it to the GPU's min().
#include <new>

#include "gs_common.h"
#include "gs_block.h"

namespace gs {

constexpr uint32_t kSortableMinInit = __builtin_bit_cast(uint32_t, 1.0e38f) ^ 0x80000000u;   // FloatToSortableUint(1.0e38)
constexpr uint32_t kSortableMaxInit = ~__builtin_bit_cast(uint32_t, -1.0e38f);              // FloatToSortableUint(-1.0e38)

// CSSelectAll (invert = 0) / CSInvertSelection (invert = 1)
__global__ __launch_bounds__(256) void edit_select_all_kernel(gsm::AssetView a, gsm::EditView e, uint32_t* __restrict__ sel, uint32_t nWords, uint32_t invert) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool cut = false;
    if (idx < a.n) {
        const gsm::V3 pos = gsm::LoadSplatPosChunk(a, idx, blockIdx.x);
        cut = gsm::IsSplatCut(e, pos.x, pos.y, pos.z);
    }
    const uint32_t cutw = ballot_word(__ballot(cut), lane);
    const uint32_t w = idx >> 5;
    if ((lane & 31u) == 0u && w < nWords) {
        uint32_t v = invert ? ~sel[w] : ~0u;
        v &= ~cutw;                                                // do not select splats that are cut
        sel[w] = v;
    }
}

// Graphics.CopyBuffer(mouse-down copy -> selected) + CSSelectionUpdate in one pass: every word is written once
__global__ __launch_bounds__(256) void edit_selection_update_kernel(gsm::AssetView a, gsm::EditView e, gsm::EditSelect S, const uint32_t* __restrict__ mouseDown,
                                                                    uint32_t* __restrict__ sel, uint32_t nWords, uint32_t add) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool hit = false;
    if (idx < a.n) hit = gsm::EditSelectionHit(S, e, gsm::LoadSplatPosChunk(a, idx, blockIdx.x));
    const uint32_t hitw = ballot_word(__ballot(hit), lane);
    const uint32_t w = idx >> 5;
    if ((lane & 31u) == 0u && w < nWords) {
        const uint32_t v = mouseDown[w];
        sel[w] = add ? (v | hitw) : (v & ~hitw);
    }
}

// gs_renderer_edit_update_selection_mask: the kernel above with the rectangle comparison replaced by the screen mask's bit under the splat's pixel
// (gsm::EditSelectionMaskHit).  The mask is at most 512 MB and typically under 1 MB: its words are read through the cache, one per hit candidate.
__global__ __launch_bounds__(256) void edit_selection_update_mask_kernel(gsm::AssetView a, gsm::EditView e, gsm::EditSelect S, gsm::MaskView M,
                                                                         const uint32_t* __restrict__ mouseDown, uint32_t* __restrict__ sel, uint32_t nWords, uint32_t add) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool hit = false;
    if (idx < a.n) hit = gsm::EditSelectionMaskHit(S, e, M, gsm::LoadSplatPosChunk(a, idx, blockIdx.x));
    const uint32_t hitw = ballot_word(__ballot(hit), lane);
    const uint32_t w = idx >> 5;
    if ((lane & 31u) == 0u && w < nWords) {
        const uint32_t v = mouseDown[w];
        sel[w] = add ? (v | hitw) : (v & ~hitw);
    }
}

// CSOrBuffers (deleted |= selected) + CSClearBuffer (selected = 0): EditDeleteSelected
__global__ __launch_bounds__(256) void edit_delete_kernel(uint32_t* __restrict__ deleted, uint32_t* __restrict__ sel, uint32_t nWords) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= nWords) return;
    deleted[w] |= sel[w];
    sel[w] = 0u;
}

// CSInitEditData
__global__ void edit_init_data_kernel(uint32_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    if (t < 9u) out[t] = t < 3u ? 0u : (t < 6u ? kSortableMinInit : kSortableMaxInit);
}

// CSUpdateEditData
__global__ __launch_bounds__(256) void edit_update_data_kernel(gsm::AssetView a, gsm::EditView e, const uint32_t* __restrict__ sel, uint32_t nWords,
                                                               uint32_t* __restrict__ out) {
    __shared__ uint32_t s_part[4][9];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool inside = idx < a.n;
    gsm::V3 pos = { 0.0f, 0.0f, 0.0f };
    bool cut = false;
    if (inside) {
        pos = gsm::LoadSplatPosChunk(a, idx, blockIdx.x);
        cut = gsm::IsSplatCut(e, pos.x, pos.y, pos.z);
    }
    const uint32_t cutw = ballot_word(__ballot(cut), lane);
    const uint32_t w = idx >> 5;
    uint32_t valSel = 0u, valDel = 0u;
    if (w < nWords) {                                              // (the 32 lanes of a word read the same address)
        valSel = sel[w];
        if (e.deletedBits) valDel = e.deletedBits[w];
    }
    valSel &= ~valDel;                                             // don't count deleted splats as selected
    valSel &= ~cutw;                                               // don't count cut splats as selected
    const uint32_t valCut = cutw & ~valDel;                        // don't count deleted splats as cut
    // counts: the popcounts of the wave's two words (held by lanes 0 and 32), bits beyond N included as in the reference
    uint32_t v[9];
    v[0] = (uint32_t)(__popc((uint32_t)__builtin_amdgcn_readlane((int)valSel, 0)) + __popc((uint32_t)__builtin_amdgcn_readlane((int)valSel, 32)));
    v[1] = (uint32_t)(__popc((uint32_t)__builtin_amdgcn_readlane((int)valDel, 0)) + __popc((uint32_t)__builtin_amdgcn_readlane((int)valDel, 32)));
    v[2] = (uint32_t)(__popc((uint32_t)__builtin_amdgcn_readlane((int)valCut, 0)) + __popc((uint32_t)__builtin_amdgcn_readlane((int)valCut, 32)));
    // bounds of the selected splats (the reference's loop stops at N: a bit beyond it has no position); a wave that selected nothing
    // -- most waves under a rectangle selection -- skips the reduction
    v[3] = v[4] = v[5] = kSortableMinInit;
    v[6] = v[7] = v[8] = kSortableMaxInit;
    const bool mine = inside && ((valSel >> (idx & 31u)) & 1u);
    if (__ballot(mine) != 0ull) {
        if (mine) gsm::EditSplatBounds(pos, v + 3, v + 6);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
            for (int k = 3; k < 6; ++k) v[k] = min(v[k], (uint32_t)__shfl_xor((int)v[k], m));
#pragma unroll
            for (int k = 6; k < 9; ++k) v[k] = max(v[k], (uint32_t)__shfl_xor((int)v[k], m));
        }
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_part[wave][k] = v[k];
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 9u) {
        const uint32_t p0 = s_part[0][t], p1 = s_part[1][t], p2 = s_part[2][t], p3 = s_part[3][t];
        if (t < 3u) {
            const uint32_t sum = p0 + p1 + p2 + p3;
            if (sum) atomicAdd(out + t, sum);
        } else if (t < 6u) {
            const uint32_t lo = min(min(p0, p1), min(p2, p3));
            if (lo != kSortableMinInit) atomicMin(out + t, lo);    // (the workgroup selected nothing: what the buffer was initialised with)
        } else {
            const uint32_t hi = max(max(p0, p1), max(p2, p3));
            if (hi != kSortableMaxInit) atomicMax(out + t, hi);
        }
    }
}

// CSTranslateSelection (OP 0), CSRotateSelection (1), CSScaleSelection (2).  The shape of the kernels above: one thread per splat, a wave owns two
// selection words; a lane reads ITS word (32 lanes, one address) and no record at an index >= N is read or written, whatever the tail bits of the
// last word say.  A wave whose two words are zero -- most waves under a rectangle selection -- leaves before it touches pos / other.  Only selected
// lanes load and store, and of a 16-byte other record only the rotation word is rewritten.  pos / other: the renderer's private blobs (null = that
// gate failed); posMD / otherMD: the mouse-down copies rotate and scale read.
//
// RIGID (gs_renderer_edit_set_rigid_transforms): the instantiations that also do what the reference's @TODOs leave out, from
// the mouse-down state like everything else here.  Rotate: the rotation word is QuatMul(q_L, rot) re-encoded and the 45 SH coefficients of the splat's
// 192-byte record go through the band matrices of L -- BakeSplatTransform's own pieces (gsm::EditRigid*), read from shMD and written to sh, the last
// 12 bytes of the record left alone.  Scale (launched for a uniform delta only): the three fp32 scales of the other record become |s| times the
// mouse-down ones; 12 bytes written.  One thread per splat, band by band: a band's 3 / 5 / 7 coefficients are loaded, multiplied out and stored before
// the next band is touched, so at most 21 + 21 coefficient registers are live and nothing spills (the resource table of section 4.15).  The band
// matrices travel by value in G, as they do into the copy kernel.  With RIGID = false the argument is an empty struct and the kernel is the text it was.
enum { kEditTranslate = 0, kEditRotate = 1, kEditScale = 2 };
struct EditNoRigid {};
struct EditRigidArgs { uint8_t* sh; const uint8_t* shMD; gsm::EditRigid G; };
template <bool RIGID> struct EditRigidArg { typedef EditNoRigid type; };
template <> struct EditRigidArg<true> { typedef EditRigidArgs type; };
template <int OP, bool RIGID = false>
__global__ __launch_bounds__(256) void edit_transform_kernel(uint8_t* __restrict__ pos, uint8_t* __restrict__ other, const uint8_t* __restrict__ posMD,
                                                             const uint8_t* __restrict__ otherMD, const uint32_t* __restrict__ sel, uint32_t n, gsm::EditXform X,
                                                             typename EditRigidArg<RIGID>::type A) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const uint32_t word = idx < n ? sel[idx >> 5] : 0u;            // idx < n: the word exists
    if (__ballot(word != 0u) == 0ull) return;
    if (!((word >> (idx & 31u)) & 1u)) return;                     // (word = 0 beyond N)
    if (pos) {
        float* dst = (float*)(pos + (size_t)idx * 12u);
        const float* src = OP == kEditTranslate ? dst : (const float*)(posMD + (size_t)idx * 12u);
        const gsm::V3 p = { src[0], src[1], src[2] };
        const gsm::V3 q = OP == kEditTranslate ? gsm::EditTranslatePos(X, p) : (OP == kEditRotate ? gsm::EditRotatePos(X, p) : gsm::EditScalePos(X, p));
        dst[0] = q.x; dst[1] = q.y; dst[2] = q.z;
    }
    if constexpr (!RIGID) {
        if (OP == kEditRotate && other) {
            const uint32_t enc = *(const uint32_t*)(otherMD + (size_t)idx * 16u);
            *(uint32_t*)(other + (size_t)idx * 16u) = gsm::EditRotateWord(X, enc);
        }
    } else if (other) {                                            // (other, sh and the three mouse-down copies exist together: the rotation gate)
        if (OP == kEditRotate) {
            const uint32_t enc = *(const uint32_t*)(otherMD + (size_t)idx * 16u);
            *(uint32_t*)(other + (size_t)idx * 16u) = gsm::EditRigidRotateWord(A.G, enc);
            gsm::EditRigidRotateSH(A.G, (const float*)(A.shMD + (size_t)idx * 192u), (float*)(A.sh + (size_t)idx * 192u));
        } else if (OP == kEditScale) {
            const float* src = (const float*)(otherMD + (size_t)idx * 16u + 4u);
            float* dst = (float*)(other + (size_t)idx * 16u + 4u);
            const gsm::V3 sc = gsm::EditRigidScale(A.G, { src[0], src[1], src[2] });
            dst[0] = sc.x; dst[1] = sc.y; dst[2] = sc.z;
        }
    }
}

// gs_renderer_edit_select_surface: one thread per pixel of the clipped rectangle.  A record counts if it carries the renderer's tag and a splat < N that
// is neither deleted nor cut (the test every kernel above makes); many pixels name the same splat and a word's splats lie anywhere in the rectangle,
// so -- unlike the kernels above, where a wave owns its words -- the bit is set or cleared with an atomic (the reference's InterlockedOr / And).
__device__ __forceinline__ void edit_select_record(const gsm::AssetView& a, const gsm::EditView& e, const gsm::PickSelect& S, const PickRecord pr,
                                                   uint32_t* __restrict__ sel) {
    if (pr.tag != S.tag || pr.splat >= a.n) return;
    const uint32_t idx = pr.splat;
    if (e.deletedBits && bit_set(e.deletedBits, idx)) return;
    const gsm::V3 pos = gsm::LoadSplatPosChunk(a, idx, idx >> 8);
    if (gsm::IsSplatCut(e, pos.x, pos.y, pos.z)) return;
    if (S.subtract) atomicAnd(sel + (idx >> 5), ~(1u << (idx & 31u)));
    else atomicOr(sel + (idx >> 5), 1u << (idx & 31u));
}

__global__ __launch_bounds__(256) void edit_select_surface_kernel(gsm::AssetView a, gsm::EditView e, gsm::PickSelect S, const PickRecord* __restrict__ rec,
                                                                  uint32_t* __restrict__ sel) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= S.w * S.h) return;
    const uint32_t x = S.x0 + i % S.w, y = S.y0 + i / S.w;
    edit_select_record(a, e, S, rec[(size_t)y * S.stride + x], sel);
}

// gs_renderer_edit_select_surface_mask: the same over the pixels whose mask bit is set.  S is the whole target (x0 = y0 = 0, w x h = the mask's size): one
// thread per pixel, 32 neighbouring lanes read one mask word, and only a pixel inside the lasso reads its record.
__global__ __launch_bounds__(256) void edit_select_surface_mask_kernel(gsm::AssetView a, gsm::EditView e, gsm::PickSelect S, gsm::MaskView M,
                                                                       const PickRecord* __restrict__ rec, uint32_t* __restrict__ sel) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;            // < 2^32: both sides are at most 65535
    if (i >= S.w * S.h) return;
    const uint32_t x = i % S.w, y = i / S.w;
    if (!gsm::MaskBit(M, x, y)) return;
    edit_select_record(a, e, S, rec[(size_t)y * S.stride + x], sel);
}

// ---- the edit history's kernels (gs_renderer_edit_checkpoint / _undo / _redo) -------------------------------------
// A checkpoint compacts the records of the selected splats into per-kind contiguous journal arrays: count, scan (export_scan_kernel), gather.  The
// shape of this file -- one thread per splat, 256-thread workgroups = one 256-splat block, a wave owns two selection words -- and the arithmetic
// (masked words, block count, rank) is gsm::Hist*, which the host harness runs too.  No atomics, no workgroup waits on another, no scratch.

// counts[b] = selected splats of block b with index < n.  Eight words and eight popcounts per block are one lane's work, so a thread takes a BLOCK (a
// workgroup per block would idle 255 of its lanes): neighbouring threads read neighbouring 32-byte runs of words.
__global__ __launch_bounds__(256) void hist_count_kernel(const uint32_t* __restrict__ sel, uint32_t nWords, uint32_t n, uint32_t blocks, uint32_t* __restrict__ counts) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= blocks) return;
    uint32_t m[8];
    gsm::HistBlockWords(sel, nWords, n, b, m);
    counts[b] = gsm::HistBlockCount(m);
}

struct HistJournal { uint32_t* idx; uint8_t* pos; uint8_t* other; uint8_t* sh; };      // k indices; k x 12 / 16 / 192 bytes (null = that kind is not captured)

// Journal slot of a selected splat = base[block] + its rank inside the block, which every wave works out for itself from the block's eight words (uniform
// loads): no wave waits for another's count.  pos / other go out per lane -- the slots of a wave's selected lanes are consecutive, so the stores of one
// instruction cover one contiguous range.  An SH record is 192 bytes: a lane copying its own record would put neighbouring lanes 192 bytes apart on both
// sides (the shape DESIGN.md section 4.8 measured slower), so a wave stages its selected INDICES in LDS (256 bytes; the rows themselves need not pass
// through LDS) and then moves the c records as c x 12 dwordx4 items, lanes striding over the items: the journal side is one contiguous, 16-byte aligned
// range, the blob side contiguous per record.  A wave whose two words are zero touches no blob.
__global__ __launch_bounds__(256) void hist_gather_kernel(const uint8_t* __restrict__ pos, const uint8_t* __restrict__ other, const uint8_t* __restrict__ sh,
                                                          const uint32_t* __restrict__ sel, uint32_t nWords, uint32_t n, const uint32_t* __restrict__ base,
                                                          HistJournal J) {
    __shared__ uint32_t s_idx[4][64];
    const uint32_t t = threadIdx.x, idx = blockIdx.x * 256u + t, lane = t & 63u, wave = t >> 6;
    uint32_t m[8];
    gsm::HistBlockWords(sel, nWords, n, blockIdx.x, m);
    const uint32_t w0 = wave == 0u ? m[0] : (wave == 1u ? m[2] : (wave == 2u ? m[4] : m[6]));
    const uint32_t w1 = wave == 0u ? m[1] : (wave == 1u ? m[3] : (wave == 2u ? m[5] : m[7]));
    if ((w0 | w1) == 0u) return;                                   // wave-uniform; no barrier below
    const uint32_t blockBase = base[blockIdx.x];
    const uint32_t waveFirst = blockBase + gsm::HistRank(m, wave * 64u);       // slot of the wave's first selected splat
    const bool mine = (((lane < 32u ? w0 : w1) >> (lane & 31u)) & 1u) != 0u;   // (masked: idx < n)
    if (mine) {
        const uint32_t slot = blockBase + gsm::HistRank(m, t);
        J.idx[slot] = idx;
        s_idx[wave][slot - waveFirst] = idx;
        if (J.pos) {
            const uint32_t* s = (const uint32_t*)(pos + (size_t)idx * 12u);
            uint32_t* d = (uint32_t*)(J.pos + (size_t)slot * 12u);
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        }
        if (J.other) *(uint4*)(J.other + (size_t)slot * 16u) = *(const uint4*)(other + (size_t)idx * 16u);
    }
    if (!J.sh) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // s_idx[wave] is this wave's own and the LDS operations of one wave complete in order:
    __builtin_amdgcn_wave_barrier();                               // nothing to wait for, the compiler only has to keep the stores above the loads
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t c = (uint32_t)(__popc(w0) + __popc(w1));
    uint4* dst = (uint4*)(J.sh + (size_t)waveFirst * 192u);
    for (uint32_t i = lane; i < c * 12u; i += 64u) {
        const uint32_t rec = i / 12u, q = i - rec * 12u;
        dst[i] = *(const uint4*)(sh + (size_t)s_idx[wave][rec] * 192u + q * 16u);
    }
}

// undo / redo: the journalled records change places with the renderer's.  The indices are distinct, so no two threads touch one record.  One thread per
// item for pos (three dwords) and other (one dwordx4 each way) ...
__global__ __launch_bounds__(256) void hist_swap_records_kernel(const uint32_t* __restrict__ idx, uint32_t k, uint8_t* __restrict__ pos, uint8_t* __restrict__ posJ,
                                                                uint8_t* __restrict__ other, uint8_t* __restrict__ otherJ) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k) return;
    const uint32_t s = idx[i];
    if (pos) {
        uint32_t* a = (uint32_t*)(pos + (size_t)s * 12u);
        uint32_t* b = (uint32_t*)(posJ + (size_t)i * 12u);
        const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
        a[0] = b0; a[1] = b1; a[2] = b2;
        b[0] = a0; b[1] = a1; b[2] = a2;
    }
    if (other) {
        uint4* a = (uint4*)(other + (size_t)s * 16u);
        uint4* b = (uint4*)(otherJ + (size_t)i * 16u);
        const uint4 va = *a, vb = *b;
        *a = vb; *b = va;
    }
}

// ... and twelve lanes per item for SH, 16 bytes each: the journal side fully contiguous, the blob side contiguous per record
__global__ __launch_bounds__(256) void hist_swap_sh_kernel(const uint32_t* __restrict__ idx, uint32_t k, uint8_t* __restrict__ sh, uint8_t* __restrict__ shJ) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= (unsigned long long)k * 12ull) return;
    const uint32_t rec = (uint32_t)(i / 12ull), q = (uint32_t)(i - (unsigned long long)rec * 12ull);
    uint4* a = (uint4*)(sh + (size_t)idx[rec] * 192u + q * 16u);
    uint4* b = (uint4*)(shJ + (size_t)i * 16u);
    const uint4 va = *a, vb = *b;
    *a = vb; *b = va;
}

// a bit buffer and its journalled copy, word for word
__global__ __launch_bounds__(256) void hist_swap_words_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint32_t nWords) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= nWords) return;
    const uint32_t va = a[w], vb = b[w];
    a[w] = vb; b[w] = va;
}

// EnsureEditingBuffers (GaussianSplatRenderer.cs:767-786) without the deleted buffer, which is made when a delete first needs it
int32_t edit_ensure(gs_renderer* r) {
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no selection: edit its owner");
    GS_HIP(hipSetDevice(r->ctx->device));
    if (r->editSelected) return GS_OK;
    const size_t bytes = bit_words(r->n) * 4;
    DevBuf<uint32_t> sel, md, cb;
    GS_HIP(sel.alloc(bytes));
    GS_HIP(md.alloc(bytes));
    GS_HIP(cb.alloc(9 * 4));
    GS_HIP(hipMemsetAsync(sel, 0, bytes, r->ctx->stream));
    GS_HIP(hipMemsetAsync(md, 0, bytes, r->ctx->stream));
    r->editSelected = std::move(sel); r->editSelectedMouseDown = std::move(md); r->editCountsBounds = std::move(cb);
    return GS_OK;
}

int32_t ensure_deleted_bits(gs_renderer* r, hipStream_t st) {
    if (r->deletedBits) return GS_OK;
    DevBuf<uint32_t> d;
    GS_HIP(d.alloc(bit_words(r->n) * 4));
    GS_HIP(hipMemsetAsync(d, 0, bit_words(r->n) * 4, st));
    r->deletedBits = std::move(d);
    return GS_OK;
}

void edit_free(gs_renderer* r) {
    r->editSelected.reset(); r->editSelectedMouseDown.reset(); r->editCountsBounds.reset();
    r->editPosMouseDown.reset(); r->editOtherMouseDown.reset(); r->editSHMouseDown.reset();
    r->editPosStored = r->editOtherStored = r->editSHStored = false;
}

static inline uint32_t splat_grid(const gs_renderer* r) { return (r->n + 255u) / 256u; }
static inline uint32_t word_grid(const gs_renderer* r) { return (uint32_t)((bit_words(r->n) + 255) / 256); }

// A 1-bit-per-splat buffer of the owner's (src) mirrored into every lane's copy of it: a device-to-device copy on each lane's OWN stream, behind
// the owner's stream -- no host synchronisation, and a frame already dealt to a lane keeps the bits of the time it was dealt (its calc_view is
// ahead of the copy on that stream).  The owner's stream then waits for the copy, so that whatever writes or frees the owner's buffer
// next (another delete, gs_renderer_set_deleted_bits) comes after the lanes have read it.
static int32_t mirror_bits_to_lanes(gs_renderer* r, const uint32_t* src, DevBuf<uint32_t> gs_renderer::* copy) {
    const size_t bytes = bit_words(r->n) * 4;
    for (gs_renderer* L : r->lanes) {
        DevBuf<uint32_t>& dst = L->*copy;
        if (!dst) GS_HIP(dst.alloc(bytes));
        GS_TRY(signal_to(r->ctx, L->ctx->stream));
        GS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, L->ctx->stream));
        GS_TRY(signal_to(L->ctx, r->ctx->stream));
    }
    return GS_OK;
}

// the lanes' copies of the deleted bits follow a delete (and an upload: gs_renderer_set_deleted_bits)
int32_t edit_deleted_to_lanes(gs_renderer* r) {
    if (r->lanes.empty()) return GS_OK;
    return mirror_bits_to_lanes(r, r->deletedBits, &gs_renderer::deletedBits);
}

// The same for the selection while it is highlighted: every call that changes editSelected ends here.  With the highlight off (or no lanes) it
// does nothing; switching the highlight on, and making lanes, bring the copies up to date (gs_api.hip).
int32_t edit_selected_to_lanes(gs_renderer* r) {
    if (r->lanes.empty() || !r->set.selectionHighlight || !r->editSelected) return GS_OK;
    return mirror_bits_to_lanes(r, r->editSelected, &gs_renderer::laneSelected);
}

// ---- the transforms ---------------------------------------------------------------------------------------------------------------------
// The reference's format gates, literally (SplatUtilities.compute:445,469,483): positions are written only in a chunk-less asset with fp32
// positions, rotation words only in a chunk-less asset with fp32 scales and fp32 SH (so an other record is 4 + 12 bytes).
static inline bool edit_pos_gate(const gs_renderer* r) { const gsm::AssetView& a = r->asset->view; return a.chunkCount == 0 && a.posFmt == 0; }
static inline bool edit_rot_gate(const gs_renderer* r) { const gsm::AssetView& a = r->asset->view; return a.chunkCount == 0 && a.scaleFmt == 0 && a.shFmt == 0; }
// what a transform may touch of blob k (0 pos, 1 other, 3 sh): whole records only
static inline size_t edit_blob_bytes(const gs_renderer* r, int k) { return (size_t)r->n * (k == 0 ? 12u : (k == 1 ? 16u : 192u)); }

// copy-on-write: the private copy of blob k (0 pos, 1 other, 2 color, 3 sh), made on the context's stream the first time a transform or a copy
// is about to write it.  Padded like an owned upload of the asset (the dword stitching of LoadUInt may touch the dword after the last record).
int32_t edit_make_private(gs_renderer* r, int k) {
    if (r->priv[k]) return GS_OK;
    const size_t bytes = (size_t)blob_bytes(r, k);
    DevBuf<uint8_t> b;
    GS_HIP(b.alloc(bytes + 16));
    GS_HIP(hipMemsetAsync(b + bytes, 0, 16, r->ctx->stream));
    GS_HIP(hipMemcpyAsync(b, blob_ptr(r, k), bytes, hipMemcpyDeviceToDevice, r->ctx->stream));
    r->priv[k] = std::move(b);
    r->privBytes[k] = bytes;
    return GS_OK;
}

// EditStorePosMouseDown / EditStoreOtherMouseDown, and the third copy the rigid rotate reads (k = 3, the SH blob: with fp32 SH -- the rotation
// gate -- a record is 192 bytes): the copy is only made where a kernel can read it (the blob's gate)
static int32_t edit_store_mouse_down(gs_renderer* r, int k) {
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    GS_HIP(hipSetDevice(r->ctx->device));
    if (k == 0 ? edit_pos_gate(r) : edit_rot_gate(r)) {
        DevBuf<uint8_t>& md = k == 0 ? r->editPosMouseDown : (k == 1 ? r->editOtherMouseDown : r->editSHMouseDown);
        if (!md) GS_HIP(md.alloc(edit_blob_bytes(r, k)));
        GS_HIP(hipMemcpyAsync(md, blob_ptr(r, k), edit_blob_bytes(r, k), hipMemcpyDeviceToDevice, r->ctx->stream));
    }
    (k == 0 ? r->editPosStored : (k == 1 ? r->editOtherStored : r->editSHStored)) = true;
    return GS_OK;
}

// the first half of the ordering described below: before the kernel that moves splats is enqueued
int32_t edit_before_move(gs_renderer* r) {
    GS_TRY(join_sort(r));
    if (vis_active(r)) GS_TRY(vis_consolidate(r));
    for (gs_renderer* L : r->lanes) GS_TRY(signal_to(L->ctx, r->ctx->stream));   // the frames dealt so far read the old positions
    return GS_OK;
}

// ... and the second: right after it
int32_t edit_after_move(gs_renderer* r) {
    GS_TRY(mark_order_use(r));
    r->movedSinceView = true;
    for (gs_renderer* L : r->lanes) L->movedSinceView = true;
    if (vis_active(r)) {
        vis_base_changed(r, r->visBaseIdentity);                   // (still CSSetIndices' identity if nothing had been sorted yet)
        GS_TRY(lanes_resync(r));
    }
    for (gs_renderer* L : r->lanes) GS_TRY(signal_to(r->ctx, L->ctx->stream));   // the kernel is behind this
    return GS_OK;
}

// One transform on the context's stream, ordered against everything else that reads the positions:
//   - a sort still running on the second queue is joined first, and the next one waits for the kernel (CSCalcDistances reads positions);
//   - GS_SORT_VISIBLE: the recorded sorts are sorts of the OLD positions, so they are carried out first (order[] = the reference's buffer now), and that
//     order is the new base with an empty history -- from here on the reference, too, stably sorts that buffer by keys of the new positions;
//   - lanes read the owner's private blobs in place: the context's stream waits for what each lane has been dealt (those frames finish with the old
//     positions), the kernel runs, and every lane's stream waits for it.  signal_to only; mirror_bits_to_lanes turned round.
// G: null = the reference's kernels; else the rigid form (the setting is on; for a scale: and the delta is uniform).
static int32_t edit_transform(gs_renderer* r, int op, const gsm::EditXform& X, const gsm::EditRigid* G = nullptr) {
    hist_transform(r);
    const bool doPos = edit_pos_gate(r), doRot = (op == kEditRotate || (G && op == kEditScale)) && edit_rot_gate(r);
    if (!doPos && !doRot) return GS_OK;                            // neither gate: the reference's kernel writes nothing
    const bool doSH = doRot && G && op == kEditRotate;
    GS_TRY(edit_before_move(r));
    if (doPos) GS_TRY(edit_make_private(r, 0));
    if (doRot) GS_TRY(edit_make_private(r, 1));
    if (doSH) GS_TRY(edit_make_private(r, 3));
    uint8_t* pos = doPos ? r->priv[0].get() : nullptr;
    uint8_t* other = doRot ? r->priv[1].get() : nullptr;
    const uint8_t* posMD = r->editPosMouseDown, * otherMD = r->editOtherMouseDown;
    const uint32_t* sel = r->editSelected;
    const dim3 grid(splat_grid(r)), block(256);
    const EditNoRigid none;
    if (G) {
        const EditRigidArgs A = { doSH ? r->priv[3].get() : nullptr, r->editSHMouseDown.get(), *G };
        if (op == kEditRotate) hipLaunchKernelGGL((edit_transform_kernel<kEditRotate, true>), grid, block, 0, r->ctx->stream, pos, other, posMD, otherMD, sel, r->n, X, A);
        else hipLaunchKernelGGL((edit_transform_kernel<kEditScale, true>), grid, block, 0, r->ctx->stream, pos, other, posMD, otherMD, sel, r->n, X, A);
    } else if (op == kEditTranslate) hipLaunchKernelGGL(edit_transform_kernel<kEditTranslate>, grid, block, 0, r->ctx->stream, pos, other, posMD, otherMD, sel, r->n, X, none);
    else if (op == kEditRotate) hipLaunchKernelGGL(edit_transform_kernel<kEditRotate>, grid, block, 0, r->ctx->stream, pos, other, posMD, otherMD, sel, r->n, X, none);
    else hipLaunchKernelGGL(edit_transform_kernel<kEditScale>, grid, block, 0, r->ctx->stream, pos, other, posMD, otherMD, sel, r->n, X, none);
    GS_HIP(hipGetLastError());
    return edit_after_move(r);
}

// ---- the edit history -----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kHistBits = GS_HIST_SELECTION | GS_HIST_DELETED;
constexpr uint32_t kHistRecords = GS_HIST_POS | GS_HIST_OTHER | GS_HIST_SH;

// entries leave a stack without a wait: they move to `dead` (no host memory for that: the stream is drained instead and they are released here)
static void hist_retire(gs_renderer* r, std::vector<EditHistEntry>& v) {
    EditHistory& h = r->hist;
    for (const EditHistEntry& e : v) h.bytes -= e.bytes;
    try {
        h.dead.reserve(h.dead.size() + v.size());
        for (EditHistEntry& e : v) h.dead.push_back(std::move(e));
    } catch (const std::bad_alloc&) {
        (void)hipStreamSynchronize(r->ctx->stream);
    }
    v.clear();
}
static void hist_drop_redo(gs_renderer* r) { if (!r->hist.redo.empty()) hist_retire(r, r->hist.redo); }

void hist_mutated(gs_renderer* r, bool selection) {
    EditHistory& h = r->hist;
    if (!h.enabled) return;
    hist_drop_redo(r);
    if (selection) ++h.selGen;
}

void hist_transform(gs_renderer* r) {
    EditHistory& h = r->hist;
    if (!h.enabled) return;
    hist_drop_redo(r);
    if (h.undo.empty() || !(h.undo.back().what & kHistRecords) || h.undo.back().selGen != h.selGen) ++h.uncovered;
}

void hist_forget(gs_renderer* r) {
    EditHistory& h = r->hist;
    if (!h.enabled) return;
    hist_drop_redo(r);
    hist_retire(r, h.undo);
    ++h.selGen;
}

// the stream has drained: nothing reads a dropped entry any more
static void hist_bury(EditHistory& h) { h.dead.clear(); }

int32_t hist_clear(gs_renderer* r) {
    EditHistory& h = r->hist;
    if (h.undo.empty() && h.redo.empty() && h.dead.empty()) return GS_OK;
    GS_HIP(hipSetDevice(r->ctx->device));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));                  // an undo's swap may still be running
    h.undo.clear(); h.redo.clear(); h.dead.clear();
    h.bytes = 0;
    return GS_OK;
}

static int32_t hist_alloc_scratch(gs_renderer* r) {
    const size_t blocks = ((size_t)r->n + 255) / 256;
    DevBuf<uint32_t> counts, base;
    if (counts.alloc(blocks * 4) != hipSuccess || base.alloc((blocks + 1) * 4) != hipSuccess) return fail(GS_ERR_OUT_OF_MEMORY, "edit history: out of device memory");
    r->hist.counts = std::move(counts); r->hist.base = std::move(base);
    return GS_OK;
}

void hist_carry(gs_renderer* to, const gs_renderer* from) {
    const EditHistory& f = from->hist;
    if (!f.enabled) return;
    if (hist_alloc_scratch(to) != GS_OK) return;                   // (no memory for two small arrays: the new state starts with the history off)
    EditHistory& t = to->hist;
    t.enabled = true; t.maxBytes = f.maxBytes; t.evicted = f.evicted; t.uncovered = f.uncovered; t.selGen = f.selGen + 1;
}

// evict the oldest entries until `extra` more bytes fit (the caller has checked that extra alone does, and has drained the stream: they are released here)
static void hist_evict_for(EditHistory& h, uint64_t extra) {
    size_t gone = 0;
    while (gone < h.undo.size() && h.bytes + extra > h.maxBytes) { h.bytes -= h.undo[gone].bytes; ++gone; ++h.evicted; }
    h.undo.erase(h.undo.begin(), h.undo.begin() + (ptrdiff_t)gone);
}

static int32_t hist_checkpoint(gs_renderer* r, uint32_t what) {
    EditHistory& h = r->hist;
    hipStream_t st = r->ctx->stream;
    GS_HIP(hipSetDevice(r->ctx->device));
    if (what & GS_HIST_TRANSFORM) what = (what & ~GS_HIST_TRANSFORM) | GS_HIST_POS | GS_HIST_OTHER | (r->set.rigidTransforms ? GS_HIST_SH : 0u);
    if (!edit_pos_gate(r)) what &= ~GS_HIST_POS;
    if (!edit_rot_gate(r)) what &= ~(GS_HIST_OTHER | GS_HIST_SH);
    if (!what) return GS_OK;
    const uint32_t nWords = (uint32_t)bit_words(r->n), blocks = splat_grid(r);
    const uint64_t bitBytes = (uint64_t)nWords * 4;
    if (what & (GS_HIST_SELECTION | kHistRecords)) GS_TRY(edit_ensure(r));
    // the count: one 4-byte readback, which also drains the stream -- whatever the dropped entries were still read by has finished
    uint32_t k = 0;
    if (what & kHistRecords) {
        hipLaunchKernelGGL(hist_count_kernel, dim3((blocks + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)r->editSelected, nWords, r->n, blocks, h.counts.get());
        GS_HIP(hipGetLastError());
        GS_TRY(enqueue_scan(st, h.counts, h.base, blocks));
        GS_HIP(hipMemcpyAsync(&k, h.base + blocks, 4, hipMemcpyDeviceToHost, st));
    }
    GS_HIP(hipStreamSynchronize(st));
    hist_bury(h);
    EditHistEntry e;
    e.what = what; e.k = k; e.selGen = h.selGen;
    const uint64_t perSplat = 4u + ((what & GS_HIST_POS) ? 12u : 0u) + ((what & GS_HIST_OTHER) ? 16u : 0u) + ((what & GS_HIST_SH) ? 192u : 0u);
    e.bytes = ((what & GS_HIST_SELECTION) ? bitBytes : 0) + ((what & GS_HIST_DELETED) ? bitBytes : 0) + ((what & kHistRecords) ? perSplat * k : 0);
    if (e.bytes > h.maxBytes) return fail(GS_ERR_OUT_OF_MEMORY, "edit checkpoint: the entry alone exceeds the history's budget");
    // everything is allocated before the stack changes.  The kernels read other / sh records as dwordx4: an asset blob the host lent at an odd address
    // becomes private (hipMalloc's alignment) first
    bool ok = true;
    if (what & GS_HIST_SELECTION) ok = ok && e.sel.alloc(bitBytes) == hipSuccess;
    if (what & GS_HIST_DELETED) ok = ok && e.del.alloc(bitBytes) == hipSuccess;
    if (k) {
        ok = ok && e.idx.alloc((size_t)k * 4) == hipSuccess;
        if (what & GS_HIST_POS) ok = ok && e.pos.alloc((size_t)k * 12) == hipSuccess;
        if (what & GS_HIST_OTHER) ok = ok && e.other.alloc((size_t)k * 16) == hipSuccess;
        if (what & GS_HIST_SH) ok = ok && e.sh.alloc((size_t)k * 192) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); return fail(GS_ERR_OUT_OF_MEMORY, "edit checkpoint: out of device memory"); }
    if (k) {
        if ((what & GS_HIST_OTHER) && ((uintptr_t)blob_ptr(r, 1) & 15u)) GS_TRY(edit_make_private(r, 1));
        if ((what & GS_HIST_SH) && ((uintptr_t)blob_ptr(r, 3) & 15u)) GS_TRY(edit_make_private(r, 3));
    }
    try { h.undo.reserve(h.undo.size() + 1); }
    catch (const std::bad_alloc&) { return fail(GS_ERR_OUT_OF_MEMORY, "edit checkpoint: out of host memory"); }
    // the captures, on the stream
    if (what & GS_HIST_SELECTION) GS_HIP(hipMemcpyAsync(e.sel, r->editSelected, bitBytes, hipMemcpyDeviceToDevice, st));
    if (what & GS_HIST_DELETED) {
        if (r->deletedBits) GS_HIP(hipMemcpyAsync(e.del, r->deletedBits, bitBytes, hipMemcpyDeviceToDevice, st));
        else GS_HIP(hipMemsetAsync(e.del, 0, bitBytes, st));      // a buffer that does not exist reads as zeros
    }
    if (k) {
        const HistJournal J = { e.idx, e.pos, e.other, e.sh };
        hipLaunchKernelGGL(hist_gather_kernel, dim3(blocks), dim3(256), 0, st, blob_ptr(r, 0), blob_ptr(r, 1), blob_ptr(r, 3), (const uint32_t*)r->editSelected,
                           nWords, r->n, (const uint32_t*)h.base, J);
        GS_HIP(hipGetLastError());
    }
    hist_drop_redo(r);
    hist_evict_for(h, e.bytes);
    h.bytes += e.bytes;
    h.undo.push_back(std::move(e));
    hist_bury(h);                                                  // nothing enqueued since the stream drained reads a dropped or evicted entry
    return GS_OK;
}

// undo (from = undo side) and redo (from = redo side): the top entry of `from` changes places with the renderer's state and moves to `to`
static int32_t hist_apply(gs_renderer* r, std::vector<EditHistEntry>& from, std::vector<EditHistEntry>& to) {
    if (from.empty()) return GS_OK;
    GS_HIP(hipSetDevice(r->ctx->device));
    try { to.reserve(to.size() + 1); } catch (const std::bad_alloc&) { return fail(GS_ERR_OUT_OF_MEMORY, "edit history: out of host memory"); }
    EditHistEntry& e = from.back();
    hipStream_t st = r->ctx->stream;
    const uint32_t nWords = (uint32_t)bit_words(r->n);
    // records: a blob without a private copy has not been written since the checkpoint (only a resize drops private copies, and it clears the history)
    uint8_t* pos = (e.what & GS_HIST_POS) && e.k ? r->priv[0].get() : nullptr;
    uint8_t* other = (e.what & GS_HIST_OTHER) && e.k ? r->priv[1].get() : nullptr;
    uint8_t* sh = (e.what & GS_HIST_SH) && e.k ? r->priv[3].get() : nullptr;
    if (pos || other || sh) {
        GS_TRY(edit_before_move(r));
        if (pos || other) hipLaunchKernelGGL(hist_swap_records_kernel, dim3((e.k + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)e.idx, e.k, pos, e.pos.get(), other, e.other.get());
        if (sh) hipLaunchKernelGGL(hist_swap_sh_kernel, dim3((uint32_t)(((uint64_t)e.k * 12u + 255u) / 256u)), dim3(256), 0, st, (const uint32_t*)e.idx, e.k, sh, e.sh.get());
        GS_HIP(hipGetLastError());
        GS_TRY(edit_after_move(r));
    }
    if (e.what & GS_HIST_DELETED) {
        GS_TRY(ensure_deleted_bits(r, st));
        hipLaunchKernelGGL(hist_swap_words_kernel, dim3(word_grid(r)), dim3(256), 0, st, r->deletedBits.get(), e.del.get(), nWords);
        GS_HIP(hipGetLastError());
        GS_TRY(edit_deleted_to_lanes(r));
    }
    if (e.what & GS_HIST_SELECTION) {
        GS_TRY(edit_ensure(r));
        hipLaunchKernelGGL(hist_swap_words_kernel, dim3(word_grid(r)), dim3(256), 0, st, r->editSelected.get(), e.sel.get(), nWords);
        GS_HIP(hipGetLastError());
        ++r->hist.selGen;
        GS_TRY(edit_selected_to_lanes(r));
    }
    to.push_back(std::move(e));
    from.pop_back();
    return GS_OK;
}

static int32_t hist_usable(const gs_renderer* r, bool needOn) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    if (needOn && !r->hist.enabled) return fail(GS_ERR_INVALID_ARGUMENT, "the edit history is off (gs_renderer_edit_history_enable)");
    return GS_OK;
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_renderer_edit_select_all(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    hipLaunchKernelGGL(edit_select_all_kernel, dim3(splat_grid(r)), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), r->editSelected,
                       (uint32_t)bit_words(r->n), 0u);
    GS_HIP(hipGetLastError());
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_invert_selection(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    hipLaunchKernelGGL(edit_select_all_kernel, dim3(splat_grid(r)), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), r->editSelected,
                       (uint32_t)bit_words(r->n), 1u);
    GS_HIP(hipGetLastError());
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_deselect_all(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    GS_HIP(hipMemsetAsync(r->editSelected, 0, bit_words(r->n) * 4, r->ctx->stream));          // CSClearBuffer
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_store_selection(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(edit_ensure(r));
    GS_HIP(hipMemcpyAsync(r->editSelectedMouseDown, r->editSelected, bit_words(r->n) * 4, hipMemcpyDeviceToDevice, r->ctx->stream));
    return GS_OK;
}

int32_t gs_renderer_edit_update_selection(gs_renderer* r, const gs_frame_params* p, const float selection_rect[4], int32_t subtract) {
    if (!r || !p || !selection_rect) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    hipLaunchKernelGGL(edit_selection_update_kernel, dim3(splat_grid(r)), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), edit_select_of(*p, selection_rect),
                       (const uint32_t*)r->editSelectedMouseDown, r->editSelected, (uint32_t)bit_words(r->n), subtract ? 0u : 1u);
    GS_HIP(hipGetLastError());
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_select_surface(gs_renderer* r, gs_target* t, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t subtract) {
    if (!r || !t) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (t->ctx != r->ctx) return fail(GS_ERR_INVALID_ARGUMENT, "target belongs to another context");
    if (!t->pick) return fail(GS_ERR_INVALID_ARGUMENT, "the target has no pick output (gs_target_set_pick_output)");
    if (x0 > x1 || y0 > y1) return fail(GS_ERR_INVALID_ARGUMENT, "select_surface: empty rectangle");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    GS_TRY(flush_clear(t));                                        // a cleared target that nothing has drawn into holds no record
    // the records' last writer: a lane's blend is joined into the context's stream by its draw, so the stream already orders this kernel after it
    const gsm::PickSelect S = pick_select_of(x0, y0, x1, y1, t->width, t->height, r->set.pickTag, subtract);
    if (S.w && S.h) {
        const uint32_t pixels = S.w * S.h;
        hipLaunchKernelGGL(edit_select_surface_kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), S,
                           (const PickRecord*)t->pick.get(), r->editSelected.get());
        GS_HIP(hipGetLastError());
        GS_TRY(target_touched(t, r->ctx->stream));
    }
    return edit_selected_to_lanes(r);                              // (counts and bounds: gs_renderer_edit_info computes them when asked, as after every selection call)
}

int32_t gs_renderer_edit_update_selection_mask(gs_renderer* r, const gs_frame_params* p, gs_mask* m, int32_t subtract) {
    if (!r || !p || !m) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (m->ctx != r->ctx) return fail(GS_ERR_INVALID_ARGUMENT, "mask belongs to another context");
    if (p->screen_w != (float)m->width || p->screen_h != (float)m->height) return fail(GS_ERR_INVALID_ARGUMENT, "update_selection_mask: the mask is not of the frame's screen size");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    const float noRect[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    const gsm::MaskView M = { m->words.get(), m->width, m->height, m->rowWords };
    hipLaunchKernelGGL(edit_selection_update_mask_kernel, dim3(splat_grid(r)), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), edit_select_of(*p, noRect), M,
                       (const uint32_t*)r->editSelectedMouseDown, r->editSelected.get(), (uint32_t)bit_words(r->n), subtract ? 0u : 1u);
    GS_HIP(hipGetLastError());
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_select_surface_mask(gs_renderer* r, gs_target* t, gs_mask* m, int32_t subtract) {
    if (!r || !t || !m) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (t->ctx != r->ctx) return fail(GS_ERR_INVALID_ARGUMENT, "target belongs to another context");
    if (m->ctx != r->ctx) return fail(GS_ERR_INVALID_ARGUMENT, "mask belongs to another context");
    if (!t->pick) return fail(GS_ERR_INVALID_ARGUMENT, "the target has no pick output (gs_target_set_pick_output)");
    if (m->width != t->width || m->height != t->height) return fail(GS_ERR_INVALID_ARGUMENT, "select_surface_mask: the mask is not of the target's size");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    GS_TRY(flush_clear(t));                                        // a cleared target that nothing has drawn into holds no record
    const gsm::PickSelect S = pick_select_of(0, 0, (int32_t)t->width - 1, (int32_t)t->height - 1, t->width, t->height, r->set.pickTag, subtract);
    const gsm::MaskView M = { m->words.get(), m->width, m->height, m->rowWords };
    const uint32_t pixels = S.w * S.h;
    hipLaunchKernelGGL(edit_select_surface_mask_kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), S, M,
                       (const PickRecord*)t->pick.get(), r->editSelected.get());
    GS_HIP(hipGetLastError());
    GS_TRY(target_touched(t, r->ctx->stream));
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_delete_selected(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(edit_ensure(r));
    GS_TRY(ensure_deleted_bits(r, r->ctx->stream));
    hist_mutated(r, true);                                         // (the delete clears the selection)
    hipLaunchKernelGGL(edit_delete_kernel, dim3(word_grid(r)), dim3(256), 0, r->ctx->stream, r->deletedBits, r->editSelected, (uint32_t)bit_words(r->n));
    GS_HIP(hipGetLastError());
    GS_TRY(edit_deleted_to_lanes(r));
    return edit_selected_to_lanes(r);                              // (the delete cleared the selection)
}

int32_t gs_renderer_edit_info(gs_renderer* r, gs_edit_info* out) {
    if (!r || !out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    memset(out, 0, sizeof(*out));
    if (!r->editSelected) return GS_OK;                            // UpdateEditCountsAndBounds without edit buffers (:707-715)
    GS_HIP(hipSetDevice(r->ctx->device));
    hipLaunchKernelGGL(edit_init_data_kernel, dim3(1), dim3(64), 0, r->ctx->stream, r->editCountsBounds);
    hipLaunchKernelGGL(edit_update_data_kernel, dim3(splat_grid(r)), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r),
                       (const uint32_t*)r->editSelected, (uint32_t)bit_words(r->n), r->editCountsBounds);
    GS_HIP(hipGetLastError());
    uint32_t res[9];
    GS_HIP(hipMemcpyAsync(res, r->editCountsBounds, sizeof(res), hipMemcpyDeviceToHost, r->ctx->stream));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));
    out->selected = res[0]; out->deleted = res[1]; out->cut = res[2];
    for (int k = 0; k < 3; ++k) {                                  // SortableUintToFloat (:699-703)
        const uint32_t lo = res[3 + k], hi = res[6 + k];
        out->bounds_min[k] = gsm::u2f(lo ^ (((lo >> 31) - 1u) | 0x80000000u));
        out->bounds_max[k] = gsm::u2f(hi ^ (((hi >> 31) - 1u) | 0x80000000u));
    }
    return GS_OK;
}

int32_t gs_renderer_edit_upload_selected_bits(gs_renderer* r, const uint32_t* words, size_t word_count) {
    if (!r || !words) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (word_count != bit_words(r->n)) return fail(GS_ERR_INVALID_ARGUMENT, "selected bits: word_count must be ceil(splat_count / 32)");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    GS_HIP(hipMemcpyAsync(r->editSelected, words, word_count * 4, hipMemcpyHostToDevice, r->ctx->stream));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));                  // `words` is only read during the call
    return edit_selected_to_lanes(r);
}

int32_t gs_renderer_edit_download_bits(gs_renderer* r, uint32_t* selected, uint32_t* selected_mouse_down, uint32_t* deleted, size_t word_count) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (word_count != bit_words(r->n)) return fail(GS_ERR_INVALID_ARGUMENT, "edit bits: word_count must be ceil(splat_count / 32)");
    GS_HIP(hipSetDevice(r->ctx->device));
    const size_t bytes = word_count * 4;
    uint32_t* const dst[3] = { selected, selected_mouse_down, deleted };
    const uint32_t* const src[3] = { r->editSelected, r->editSelectedMouseDown, r->deletedBits };
    for (int k = 0; k < 3; ++k) {
        if (!dst[k]) continue;
        if (src[k]) GS_HIP(hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyDeviceToHost, r->ctx->stream));
        else memset(dst[k], 0, bytes);                             // a buffer that does not exist reads as zeros
    }
    GS_HIP(hipStreamSynchronize(r->ctx->stream));
    return GS_OK;
}

int32_t gs_renderer_edit_store_pos_mouse_down(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    return edit_store_mouse_down(r, 0);
}

int32_t gs_renderer_edit_store_other_mouse_down(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    return edit_store_mouse_down(r, 1);
}

int32_t gs_renderer_edit_store_sh_mouse_down(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    return edit_store_mouse_down(r, 3);
}

int32_t gs_renderer_edit_set_rigid_transforms(gs_renderer* r, int32_t enabled) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane has no settings of its own: set its owner's");
    r->set.rigidTransforms = enabled != 0;
    return GS_OK;
}

int32_t gs_renderer_edit_translate_selection(gs_renderer* r, const float delta[3]) {
    if (!r || !delta) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_TRY(edit_ensure(r));
    return edit_transform(r, kEditTranslate, edit_xform_of(nullptr, nullptr, nullptr, delta, 3));
}

int32_t gs_renderer_edit_rotate_selection(gs_renderer* r, const float center[3], const float local_to_world[16], const float world_to_local[16],
                                          const float rotation_xyzw[4]) {
    if (!r || !center || !local_to_world || !world_to_local || !rotation_xyzw) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_TRY(edit_ensure(r));
    if (!r->editPosStored || !r->editOtherStored)                  // "should have captured initial state" (:859)
        return fail(GS_ERR_INVALID_ARGUMENT, "rotate: the mouse-down copies of pos and other have not been stored");
    const gsm::EditXform X = edit_xform_of(center, local_to_world, world_to_local, rotation_xyzw, 4);
    if (!r->set.rigidTransforms) return edit_transform(r, kEditRotate, X);
    if (!r->editSHStored) return fail(GS_ERR_INVALID_ARGUMENT, "rigid rotate: the mouse-down copy of sh has not been stored");
    gsm::EditRigid G;
    float L[12];
    if (const char* why = edit_rigid_rotate_of(local_to_world, world_to_local, rotation_xyzw, G, L)) return fail(GS_ERR_INVALID_ARGUMENT, why);
    return edit_transform(r, kEditRotate, X, &G);
}

int32_t gs_renderer_edit_scale_selection(gs_renderer* r, const float center[3], const float local_to_world[16], const float world_to_local[16],
                                         const float scale[3]) {
    if (!r || !center || !local_to_world || !world_to_local || !scale) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_TRY(edit_ensure(r));
    if (!r->editPosStored) return fail(GS_ERR_INVALID_ARGUMENT, "scale: the mouse-down copy of pos has not been stored");      // :880
    const gsm::EditXform X = edit_xform_of(center, local_to_world, world_to_local, scale, 3);
    if (!r->set.rigidTransforms || !edit_rigid_scale_uniform(scale)) return edit_transform(r, kEditScale, X);
    if (!r->editOtherStored) return fail(GS_ERR_INVALID_ARGUMENT, "rigid scale: the mouse-down copy of other has not been stored");
    const gsm::EditRigid G = edit_rigid_scale_of(scale);
    return edit_transform(r, kEditScale, X, &G);
}

int32_t gs_renderer_edit_download_pos_other(gs_renderer* r, void* pos, size_t pos_bytes, void* other, size_t other_bytes) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if ((pos && pos_bytes > blob_bytes(r, 0)) || (other && other_bytes > blob_bytes(r, 1))) return fail(GS_ERR_INVALID_ARGUMENT, "more bytes asked for than the blob holds");
    GS_HIP(hipSetDevice(r->ctx->device));
    if (pos && pos_bytes) GS_HIP(hipMemcpyAsync(pos, blob_ptr(r, 0), pos_bytes, hipMemcpyDeviceToHost, r->ctx->stream));
    if (other && other_bytes) GS_HIP(hipMemcpyAsync(other, blob_ptr(r, 1), other_bytes, hipMemcpyDeviceToHost, r->ctx->stream));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));
    return GS_OK;
}

int32_t gs_renderer_edit_release(gs_renderer* r) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (!r->editSelected && !r->editPosStored && !r->editOtherStored && !r->editSHStored) return GS_OK;
    GS_HIP(hipSetDevice(r->ctx->device));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));
    for (gs_renderer* L : r->lanes) {                              // no edit buffers, nothing to highlight: the lanes' copies go once their frames have read them
        if (!L->laneSelected) continue;
        GS_HIP(hipStreamSynchronize(L->ctx->stream));
        L->laneSelected.reset();
    }
    edit_free(r);
    return GS_OK;
}

int32_t gs_renderer_edit_history_enable(gs_renderer* r, uint64_t max_bytes) {
    GS_TRY(hist_usable(r, false));
    EditHistory& h = r->hist;
    if (max_bytes == 0) {
        GS_TRY(hist_clear(r));
        if (h.enabled) { GS_HIP(hipSetDevice(r->ctx->device)); GS_HIP(hipStreamSynchronize(r->ctx->stream)); }   // (a checkpoint's count may be the last thing enqueued)
        h.counts.reset(); h.base.reset();
        h.enabled = false; h.maxBytes = 0; h.evicted = h.uncovered = 0; h.selGen = 0;
        return GS_OK;
    }
    GS_HIP(hipSetDevice(r->ctx->device));
    if (!h.enabled) {
        GS_TRY(hist_alloc_scratch(r));
        h.enabled = true; h.evicted = h.uncovered = 0; h.selGen = 0; h.bytes = 0;
    }
    h.maxBytes = max_bytes;
    if (h.bytes > h.maxBytes) {                                    // a smaller budget: the oldest undo entries go first, then the farthest redo entries
        GS_HIP(hipStreamSynchronize(r->ctx->stream));
        hist_evict_for(h, 0);
        while (!h.redo.empty() && h.bytes > h.maxBytes) { h.bytes -= h.redo.front().bytes; h.redo.erase(h.redo.begin()); ++h.evicted; }
        hist_bury(h);
    }
    return GS_OK;
}

int32_t gs_renderer_edit_checkpoint(gs_renderer* r, uint32_t what) {
    GS_TRY(hist_usable(r, true));
    if (what == 0u || (what & ~(kHistBits | kHistRecords | GS_HIST_TRANSFORM))) return fail(GS_ERR_INVALID_ARGUMENT, "edit checkpoint: `what` is zero or has unknown bits");
    return hist_checkpoint(r, what);
}

int32_t gs_renderer_edit_undo(gs_renderer* r) {
    GS_TRY(hist_usable(r, true));
    return hist_apply(r, r->hist.undo, r->hist.redo);
}

int32_t gs_renderer_edit_redo(gs_renderer* r) {
    GS_TRY(hist_usable(r, true));
    return hist_apply(r, r->hist.redo, r->hist.undo);
}

int32_t gs_renderer_edit_history_clear(gs_renderer* r) {
    GS_TRY(hist_usable(r, false));
    return hist_clear(r);
}

int32_t gs_renderer_edit_history_info(const gs_renderer* r, gs_edit_history_info* out) {
    GS_TRY(hist_usable(r, false));
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    memset(out, 0, sizeof(*out));
    const EditHistory& h = r->hist;
    out->enabled = h.enabled ? 1u : 0u;
    out->undo_depth = (uint32_t)h.undo.size(); out->redo_depth = (uint32_t)h.redo.size();
    out->bytes = h.bytes; out->max_bytes = h.maxBytes;
    if (!h.undo.empty()) { out->top_what = h.undo.back().what; out->top_bytes = h.undo.back().bytes; out->top_splats = h.undo.back().k; }
    out->evicted = h.evicted; out->uncovered_transforms = h.uncovered;
    return GS_OK;
}

} // extern "C"
