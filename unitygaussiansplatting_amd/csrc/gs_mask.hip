// gs_mask.hip -- the screen mask of the lasso, polygon and brush tools: one bit per pixel, drawn on the GPU (gs_mask_*).
// What a pixel's bit is after a drawing call is defined operation by operation in include/gsplat_c.h; the arithmetic is gsm::Mask* (gs_device_math.h),
// which the host harness runs too.  The two calls that select THROUGH a mask are in gs_edit.hip, beside the rectangle kernels.
//
// mask_polygon_kernel -- a 256-thread workgroup per ROW.  Parity is an XOR, so the edges may be taken in any order and grouping:
//   1. the edges go through the workgroup in batches of kMaskEdgeBatch = 256, one edge per thread (neighbouring threads read neighbouring vertices).  An
//      edge that crosses the row's centre line is reduced to k = gsm::MaskBoundaryCount(xs, W), the number of pixels left of the crossing -- pixels
//      0 .. k-1 are toggled -- and leaves ONE LDS atomicXor, at bit k - 1 of the row's toggle words (k = 0 toggles nothing);
//   2. pixel x is covered iff an odd number of toggle bits lie at or above x: a suffix parity.  Inside a word by shift-XOR doubling (five steps); across
//      words the parity of each word's total travels through one __ballot per wave (a lane XORs the popcount of the lanes above it) and four LDS words
//      per workgroup, 256 words per round from the top of the row down, a carry bit between rounds (one round up to W = 8192);
//   3. one word load, OR / AND-NOT, one word store per 32 pixels.  A word whose coverage is zero is not touched.  No global atomics: a workgroup owns its row.
// mask_stroke_kernel -- a 256-thread workgroup per SEGMENT, over the segment's conservative pixel box (gsm::MaskSegmentBox) widened to whole 64-pixel
// groups: a wave takes a row of a group at a time, a lane a pixel; the 64 verdicts become two words through __ballot and the two lanes that own them
// leave at most one global atomicOr (subtract: atomicAnd) each, none for a word nothing covers.  Segments overlap, so here a word has many writers and the
// atomic is needed; OR and AND-NOT commute, so the result does not depend on their order.  The work is the pixels of the boxes, not W x H x P.
#include <new>

#include "gs_common.h"

namespace gs {

constexpr uint32_t kMaskEdgeBatch = 256;
constexpr uint32_t kMaskMaxRowWords = 2048;                        // ceil(65535 / 32)

__global__ __launch_bounds__(256) void mask_polygon_kernel(uint32_t* __restrict__ words, uint32_t w, uint32_t rowWords, const float2* __restrict__ v, uint32_t count,
                                                           uint32_t subtract) {
    __shared__ uint32_t s_tog[kMaskMaxRowWords];
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, y = blockIdx.x;
    for (uint32_t i = t; i < rowWords; i += 256u) s_tog[i] = 0u;
    __syncthreads();
    const float yc = (float)y + 0.5f;
    for (uint32_t base = 0; base < count; base += kMaskEdgeBatch) {
        const uint32_t i = base + t;
        if (i >= count) continue;
        const float2 a = v[i], b = v[i + 1u == count ? 0u : i + 1u];
        if (!gsm::MaskEdgeCrosses(a.y, b.y, yc)) continue;
        const uint32_t k = gsm::MaskBoundaryCount(gsm::MaskEdgeCrossX(a.x, a.y, b.x, b.y, yc), w);     // 0 .. w
        if (k) atomicXor(&s_tog[(k - 1u) >> 5], 1u << ((k - 1u) & 31u));                              // (k - 1) >> 5 < rowWords
    }
    __syncthreads();
    uint32_t* row = words + (size_t)y * rowWords;
    const uint32_t rounds = (rowWords + 255u) / 256u;
    uint32_t carry = 0u;                                           // parity of every toggle bit above the current round's words
    for (uint32_t r = rounds; r-- > 0u;) {
        const uint32_t wi = r * 256u + t;
        uint32_t s = wi < rowWords ? s_tog[wi] : 0u;
        s ^= s >> 1; s ^= s >> 2; s ^= s >> 4; s ^= s >> 8; s ^= s >> 16;      // bit j = parity of the word's bits j .. 31; bit 0 = of the whole word
        const unsigned long long odd = __ballot(s & 1u);
        const uint32_t above = lane == 63u ? 0u : (uint32_t)__popcll(odd >> (lane + 1u));            // odd words in the lanes above this one
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(odd);
        __syncthreads();
        uint32_t higher = carry + above, all = carry;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t c = s_wave[k];
            all += c;
            if (k > wave) higher += c;
        }
        __syncthreads();                                           // s_wave is written again in the next round
        carry = all & 1u;
        if (wi < rowWords) {
            uint32_t cov = (higher & 1u) ? ~s : s;
            if (wi == rowWords - 1u) cov &= gsm::MaskTailBits(w);
            if (cov) row[wi] = subtract ? (row[wi] & ~cov) : (row[wi] | cov);
        }
    }
}

__global__ __launch_bounds__(256) void mask_stroke_kernel(uint32_t* __restrict__ words, uint32_t w, uint32_t h, uint32_t rowWords, const float2* __restrict__ p,
                                                          uint32_t points, float radius, uint32_t subtract) {
    const uint32_t seg = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float2 a = p[seg], b = p[seg + 1u < points ? seg + 1u : seg];       // (one point: the segment a -> a)
    const gsm::MaskBox B = gsm::MaskSegmentBox(a.x, a.y, b.x, b.y, radius, w, h);
    if (B.x0 > B.x1 || B.y0 > B.y1) return;                        // nothing of the box on screen (0 <= x0, x1 < w, 0 <= y0, y1 < h otherwise)
    const float r2 = radius * radius;
    const uint32_t g0 = (uint32_t)B.x0 >> 6, groups = ((uint32_t)B.x1 >> 6) - g0 + 1u, rows = (uint32_t)(B.y1 - B.y0) + 1u;
    const uint32_t items = groups * rows;                          // <= 1024 x 65535
    for (uint32_t it = wave; it < items; it += 4u) {               // wave-uniform
        const uint32_t y = (uint32_t)B.y0 + it / groups, x = ((g0 + it % groups) << 6) + lane;
        const bool in = x < w && gsm::MaskSegmentCovers(a.x, a.y, b.x, b.y, (float)x + 0.5f, (float)y + 0.5f, r2);
        const unsigned long long m = __ballot(in);
        const uint32_t mine = (uint32_t)(m >> (lane & 32u));
        if ((lane & 31u) == 0u && mine) {                          // mine != 0: a pixel x' < w of this word is covered, so the word exists
            uint32_t* dst = words + (size_t)y * rowWords + (x >> 5);
            if (subtract) atomicAnd(dst, ~mine); else atomicOr(dst, mine);
        }
    }
}

// the bits beyond W of every row's last word, after an upload
__global__ __launch_bounds__(256) void mask_trim_kernel(uint32_t* __restrict__ words, uint32_t h, uint32_t rowWords, uint32_t tail) {
    const uint32_t y = blockIdx.x * 256u + threadIdx.x;
    if (y < h) words[(size_t)y * rowWords + rowWords - 1u] &= tail;
}

static inline size_t mask_words(const gs_mask* m) { return (size_t)m->height * m->rowWords; }

// the caller's points become the mask's device copy, through the pinned shadow; refuses what the header says
static int32_t mask_stage_points(gs_mask* m, const float* xy, uint32_t count) {
    for (size_t i = 0; i < (size_t)count * 2; ++i)
        if (!gsm::MaskCoordOk(xy[i])) return fail(GS_ERR_INVALID_ARGUMENT, "mask: a coordinate is NaN, infinite or beyond 65536 in magnitude");
    GS_HIP(hipSetDevice(m->ctx->device));
    if (count > m->xyCap) {
        uint32_t cap = 1024;
        while (cap < count) cap <<= 1;
        if (m->xyCopyPending) GS_HIP(hipEventSynchronize(m->xyCopied));
        GS_HIP(hipStreamSynchronize(m->ctx->stream));             // a kernel may still read the smaller copy
        DevBuf<float> dev; PinnedBuf<float> host;
        GS_HIP(dev.alloc((size_t)cap * 8));
        GS_HIP(host.alloc((size_t)cap * 8, hipHostMallocDefault));
        if (!m->xyCopied) GS_HIP(m->xyCopied.create(hipEventDisableTiming));
        m->xy = std::move(dev); m->xyHost = std::move(host);
        m->xyCap = cap; m->xyCopyPending = false;
    }
    if (m->xyCopyPending) GS_HIP(hipEventSynchronize(m->xyCopied));   // the shadow is still being read
    memcpy(m->xyHost, xy, (size_t)count * 8);
    GS_HIP(hipMemcpyAsync(m->xy, m->xyHost, (size_t)count * 8, hipMemcpyHostToDevice, m->ctx->stream));
    GS_HIP(hipEventRecord(m->xyCopied, m->ctx->stream));
    m->xyCopyPending = true;
    return GS_OK;
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_mask_create(gs_context* ctx, uint32_t w, uint32_t h, gs_mask** out) {
    if (!ctx || !out || w == 0 || h == 0 || w > 65535 || h > 65535) return fail(GS_ERR_INVALID_ARGUMENT, "bad argument");
    *out = nullptr;
    GS_HIP(hipSetDevice(ctx->device));
    gs_mask* m = new (std::nothrow) gs_mask();
    if (!m) return fail(GS_ERR_OUT_OF_MEMORY, "host allocation");
    m->ctx = ctx; m->width = w; m->height = h; m->rowWords = gsm::MaskRowWords(w);
    hipError_t e = m->words.alloc(mask_words(m) * 4);
    if (e == hipSuccess) e = hipMemsetAsync(m->words, 0, mask_words(m) * 4, ctx->stream);
    if (e != hipSuccess) { delete m; return fail_hip(e, "alloc mask", __FILE__, __LINE__); }
    *out = m;
    return GS_OK;
}

int32_t gs_mask_destroy(gs_mask* m) {
    if (!m) return GS_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    delete m;
    return GS_OK;
}

int32_t gs_mask_clear(gs_mask* m) {
    if (!m) return fail(GS_ERR_INVALID_ARGUMENT, "mask is null");
    GS_HIP(hipSetDevice(m->ctx->device));
    GS_HIP(hipMemsetAsync(m->words, 0, mask_words(m) * 4, m->ctx->stream));
    return GS_OK;
}

int32_t gs_mask_upload(gs_mask* m, const uint32_t* words, size_t word_count) {
    if (!m || !words) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (word_count != mask_words(m)) return fail(GS_ERR_INVALID_ARGUMENT, "mask: word_count must be height * ceil(width / 32)");
    GS_HIP(hipSetDevice(m->ctx->device));
    if (!m->wordsHost) {                                           // both resources or neither
        PinnedBuf<uint32_t> host; Event ev;
        GS_HIP(host.alloc(word_count * 4, hipHostMallocDefault));
        GS_HIP(ev.create(hipEventDisableTiming));
        m->wordsHost = std::move(host); m->wordsCopied = std::move(ev);
    }
    if (m->wordsCopyPending) GS_HIP(hipEventSynchronize(m->wordsCopied));    // the shadow is still being read
    memcpy(m->wordsHost, words, word_count * 4);                   // `words` is only read during the call
    GS_HIP(hipMemcpyAsync(m->words, m->wordsHost, word_count * 4, hipMemcpyHostToDevice, m->ctx->stream));
    GS_HIP(hipEventRecord(m->wordsCopied, m->ctx->stream));
    m->wordsCopyPending = true;
    if (m->width & 31u) {
        hipLaunchKernelGGL(mask_trim_kernel, dim3((m->height + 255u) / 256u), dim3(256), 0, m->ctx->stream, m->words.get(), m->height, m->rowWords, gsm::MaskTailBits(m->width));
        GS_HIP(hipGetLastError());
    }
    return GS_OK;
}

int32_t gs_mask_download(gs_mask* m, uint32_t* words, size_t word_count) {
    if (!m || !words) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (word_count != mask_words(m)) return fail(GS_ERR_INVALID_ARGUMENT, "mask: word_count must be height * ceil(width / 32)");
    GS_HIP(hipSetDevice(m->ctx->device));
    GS_HIP(hipMemcpyAsync(words, m->words, word_count * 4, hipMemcpyDeviceToHost, m->ctx->stream));
    GS_HIP(hipStreamSynchronize(m->ctx->stream));
    return GS_OK;
}

int32_t gs_mask_fill_polygon(gs_mask* m, const float* xy, uint32_t vertices, int32_t subtract) {
    if (!m || !xy) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (vertices < 3u || vertices > gsm::kMaskMaxPoints) return fail(GS_ERR_INVALID_ARGUMENT, "mask: a polygon has 3 .. 65536 vertices");
    GS_TRY(mask_stage_points(m, xy, vertices));
    hipLaunchKernelGGL(mask_polygon_kernel, dim3(m->height), dim3(256), 0, m->ctx->stream, m->words.get(), m->width, m->rowWords, (const float2*)m->xy.get(), vertices,
                       subtract ? 1u : 0u);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

int32_t gs_mask_stroke(gs_mask* m, const float* xy, uint32_t points, float radius, int32_t subtract) {
    if (!m || !xy) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (points < 1u || points > gsm::kMaskMaxPoints) return fail(GS_ERR_INVALID_ARGUMENT, "mask: a stroke has 1 .. 65536 points");
    if (!(radius > 0.0f && radius <= gsm::kMaskCoordMax)) return fail(GS_ERR_INVALID_ARGUMENT, "mask: the radius must be in (0, 65536]");
    GS_TRY(mask_stage_points(m, xy, points));
    hipLaunchKernelGGL(mask_stroke_kernel, dim3(points > 1u ? points - 1u : 1u), dim3(256), 0, m->ctx->stream, m->words.get(), m->width, m->height, m->rowWords,
                       (const float2*)m->xy.get(), points, radius, subtract ? 1u : 0u);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

} // extern "C"
