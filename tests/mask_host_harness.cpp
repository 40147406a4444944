// Test-only: the screen mask's arithmetic (csrc/gs_device_math.h: gsm::Mask*, EditSelectionMaskHit) compiled for the HOST and run the way the kernels of
// gs_mask.hip run it -- per row the crossings reduced to boundary counts, one XOR per crossing, a suffix parity; per segment the pixels of its conservative
// box -- so that tests/test_mask_host.py can hold it to the brute-force twin of tests/mask_model.py bit for bit on a box without a GPU.  Never shipped.
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {

uint32_t mh_boundary_count(float xs, uint32_t w) { return gsm::MaskBoundaryCount(xs, w); }

// words: h x ceil(w/32), read and written (set or subtract), as gs_mask_fill_polygon leaves them
void mh_fill_polygon(uint32_t w, uint32_t h, const float* xy, uint32_t count, int32_t subtract, uint32_t* words) {
    const uint32_t rowWords = gsm::MaskRowWords(w);
    std::vector<uint32_t> tog(rowWords);
    for (uint32_t y = 0; y < h; ++y) {
        std::fill(tog.begin(), tog.end(), 0u);
        const float yc = (float)y + 0.5f;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t j = i + 1u == count ? 0u : i + 1u;
            const float ax = xy[2 * i], ay = xy[2 * i + 1], bx = xy[2 * j], by = xy[2 * j + 1];
            if (!gsm::MaskEdgeCrosses(ay, by, yc)) continue;
            const uint32_t k = gsm::MaskBoundaryCount(gsm::MaskEdgeCrossX(ax, ay, bx, by, yc), w);
            if (k) tog[(k - 1u) >> 5] ^= 1u << ((k - 1u) & 31u);
        }
        uint32_t carry = 0u;
        for (uint32_t wi = rowWords; wi-- > 0u;) {
            uint32_t s = tog[wi];
            s ^= s >> 1; s ^= s >> 2; s ^= s >> 4; s ^= s >> 8; s ^= s >> 16;
            uint32_t cov = carry ? ~s : s;
            carry ^= s & 1u;
            if (wi == rowWords - 1u) cov &= gsm::MaskTailBits(w);
            uint32_t& dst = words[(size_t)y * rowWords + wi];
            dst = subtract ? (dst & ~cov) : (dst | cov);
        }
    }
}

// returns the number of pixel tests made (the boxes' pixels, not w * h * segments)
uint64_t mh_stroke(uint32_t w, uint32_t h, const float* xy, uint32_t points, float radius, int32_t subtract, uint32_t* words) {
    const uint32_t rowWords = gsm::MaskRowWords(w), segments = points > 1u ? points - 1u : 1u;
    const float r2 = radius * radius;
    uint64_t tests = 0;
    for (uint32_t s = 0; s < segments; ++s) {
        const uint32_t e = s + 1u < points ? s + 1u : s;
        const float ax = xy[2 * s], ay = xy[2 * s + 1], bx = xy[2 * e], by = xy[2 * e + 1];
        const gsm::MaskBox B = gsm::MaskSegmentBox(ax, ay, bx, by, radius, w, h);
        for (int32_t y = B.y0; y <= B.y1; ++y)
            for (int32_t x = B.x0; x <= B.x1; ++x) {
                ++tests;
                if (!gsm::MaskSegmentCovers(ax, ay, bx, by, (float)x + 0.5f, (float)y + 0.5f, r2)) continue;
                uint32_t& dst = words[(size_t)y * rowWords + ((uint32_t)x >> 5)];
                const uint32_t bit = 1u << ((uint32_t)x & 31u);
                dst = subtract ? (dst & ~bit) : (dst | bit);
            }
    }
    return tests;
}

// hit[i] of gs_renderer_edit_update_selection_mask over n fp32 positions (a chunk-less asset's pos blob)
void mh_selection_hits(const float* pos, uint32_t n, const gs_frame_params* p, const gs_cutout* cutouts, uint32_t cutoutCount, const uint32_t* words, uint32_t w,
                       uint32_t h, uint8_t* hit) {
    gsm::EditView e; e.deletedBits = nullptr; e.cutouts = (const uint32_t*)cutouts; e.cutoutCount = cutoutCount;
    const float noRect[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    const gsm::EditSelect S = gs::edit_select_of(*p, noRect);
    const gsm::MaskView M = { words, w, h, gsm::MaskRowWords(w) };
    for (uint32_t i = 0; i < n; ++i) hit[i] = gsm::EditSelectionMaskHit(S, e, M, { pos[3 * i], pos[3 * i + 1], pos[3 * i + 2] }) ? 1 : 0;
}

int32_t mh_coord_ok(float v) { return gsm::MaskCoordOk(v) ? 1 : 0; }

}
