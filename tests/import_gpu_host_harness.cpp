// Test-only: the arithmetic of the GPU import (csrc/gs_device_math.h: gsm::ImportExpDet, gsm::ImportLinearize, gsm::ImportRecord, the BC7 mode-6 block
// encoder gsm::BC7* in its one-thread and its sixteen-lane form, and the whole pipeline run serially: ImportRecord -> bounds -> Morton order -> the
// Bake* chunk encode) compiled for the HOST, so that tests/test_import_gpu_model.py can hold it to the native importer (gs_import_encode) byte for byte
// on a box without a GPU.  Never part of the shipped library.  With -DIMPORT_GPU_HARNESS_MAIN it is a stand-alone program (its own main) that runs
// every entry point over a small input it makes itself, the blobs at the importer's exact sizes: the form a sanitizer build runs.
#include <algorithm>
#include <numeric>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

namespace {

// the records of splats [0, n) in destination order (Morton order of their positions when asked for), and the position bounds
std::vector<gsm::BakeRec> ordered_records(const gsm::ImportSrc& in, uint32_t n, uint32_t linearize, uint32_t morton, float* bounds) {
    std::vector<gsm::BakeRec> rec(n);
    for (uint32_t j = 0; j < n; ++j) gsm::ImportRecord(in, j, linearize, rec[j]);
    const float inf = gsm::u2f(0x7f800000u);
    for (int c = 0; c < 3; ++c) { bounds[c] = inf; bounds[3 + c] = -inf; }
    for (uint32_t j = 0; j < n; ++j) {
        const float p[3] = { rec[j].pos.x, rec[j].pos.y, rec[j].pos.z };
        for (int c = 0; c < 3; ++c) { bounds[c] = fminf(bounds[c], p[c]); bounds[3 + c] = fmaxf(bounds[3 + c], p[c]); }
    }
    if (!morton) return rec;
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::vector<uint64_t> code(n);
    for (uint32_t j = 0; j < n; ++j) code[j] = gsm::BakeMortonCode(rec[j].pos, bounds, bounds + 3);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return code[x] < code[y]; });      // (code, index)
    std::vector<gsm::BakeRec> out(n);
    for (uint32_t j = 0; j < n; ++j) out[j] = rec[order[j]];
    return out;
}

// what one DPP step of the kernel's row reduction hands lane l: the value of lane l ^ 1, l ^ 2, 7 - l inside its half, 15 - l
uint32_t row_partner(uint32_t l, int step) { return step == 0 ? l ^ 1u : (step == 1 ? l ^ 2u : (step == 2 ? (l & 8u) | (7u - (l & 7u)) : 15u - l)); }

} // namespace

extern "C" {
void igh_exp(const float* x, uint32_t n, float* out) { for (uint32_t i = 0; i < n; ++i) out[i] = gsm::ImportExpDet(x[i]); }

// the linearised fields of every splat: dc0 3, scale 3, opacity 1, rot 4 -> lin[n][11]; word[n] = ImportRecord's rotation word
void igh_linearize(const gsm::ImportSrc* in, uint32_t n, uint32_t linearize, float* lin, uint32_t* word) {
    for (uint32_t i = 0; i < n; ++i) {
        gsm::V3 dc0 = { in->dc0[i * 3], in->dc0[i * 3 + 1], in->dc0[i * 3 + 2] }, scale = { in->scale[i * 3], in->scale[i * 3 + 1], in->scale[i * 3 + 2] };
        float opacity = in->opacity[i];
        gsm::V4 rot = { in->rot[i * 4], in->rot[i * 4 + 1], in->rot[i * 4 + 2], in->rot[i * 4 + 3] };
        if (linearize) gsm::ImportLinearize(dc0, scale, opacity, rot);
        const float v[11] = { dc0.x, dc0.y, dc0.z, scale.x, scale.y, scale.z, opacity, rot.x, rot.y, rot.z, rot.w };
        memcpy(lin + (size_t)i * 11, v, sizeof(v));
        gsm::BakeRec rec;
        gsm::ImportRecord(*in, i, linearize, rec);
        word[i] = rec.rot;
    }
}

// nb blocks of 16 texels (row-major in the block) x RGBA in 0..1 as the colour texture holds them -> 16 bytes each, one thread per block.
// flags[b]: bit 0 = the anchor flip happened, bit 1 / 2 = the p-bit of the low / high endpoint as quantised (before the flip)
void igh_bc7_blocks(const float* texels, uint32_t nb, uint8_t* out, uint32_t* flags) {
    for (uint32_t b = 0; b < nb; ++b) {
        float px[16][4];
        for (int t = 0; t < 16; ++t) { const float* s = texels + ((size_t)b * 16 + t) * 4; gsm::BC7Texel({ s[0], s[1], s[2], s[3] }, px[t]); }
        uint32_t w[4];
        gsm::BC7EncodeMode6(px, w);
        gsm::BakeStoreBytes(out + (size_t)b * 16, w, 16u);
        float lo[4], hi[4];
        for (int c = 0; c < 4; ++c) { lo[c] = hi[c] = px[0][c]; for (int t = 1; t < 16; ++t) { lo[c] = fminf(lo[c], px[t][c]); hi[c] = fmaxf(hi[c], px[t][c]); } }
        gsm::BC7Block blk;
        gsm::BC7Endpoints(lo, hi, blk);
        flags[b] = (gsm::BC7TexelIndex(blk, px[0]) >= 8u ? 1u : 0u) | ((uint32_t)blk.p0 << 1) | ((uint32_t)blk.p1 << 2);
    }
}

// the same blocks the way bake_encode_kernel makes them, emulated lane by lane: lane l of a row of sixteen holds texel BC7TexelOfLane(l); the four
// exchange steps of the row reduction for the minima, the maxima and the gathered indices; the endpoints per lane; the pack by the row's first lane
void igh_bc7_blocks_lanes(const float* texels, uint32_t nb, uint8_t* out) {
    for (uint32_t b = 0; b < nb; ++b) {
        float px[16][4], lo[16][4], hi[16][4];
        for (uint32_t l = 0; l < 16u; ++l) {
            const float* s = texels + ((size_t)b * 16 + gsm::BC7TexelOfLane(l)) * 4;
            gsm::BC7Texel({ s[0], s[1], s[2], s[3] }, px[l]);
            for (int c = 0; c < 4; ++c) lo[l][c] = hi[l][c] = px[l][c];
        }
        for (int step = 0; step < 4; ++step) {
            float lo2[16][4], hi2[16][4];
            for (uint32_t l = 0; l < 16u; ++l)
                for (int c = 0; c < 4; ++c) { lo2[l][c] = fminf(lo[l][c], lo[row_partner(l, step)][c]); hi2[l][c] = fmaxf(hi[l][c], hi[row_partner(l, step)][c]); }
            memcpy(lo, lo2, sizeof(lo)); memcpy(hi, hi2, sizeof(hi));
        }
        uint64_t nib[16];
        gsm::BC7Block blk[16];
        for (uint32_t l = 0; l < 16u; ++l) {
            gsm::BC7Endpoints(lo[l], hi[l], blk[l]);
            nib[l] = (uint64_t)gsm::BC7TexelIndex(blk[l], px[l]) << (4u * gsm::BC7TexelOfLane(l));
        }
        for (int step = 0; step < 4; ++step) {
            uint64_t nib2[16];
            for (uint32_t l = 0; l < 16u; ++l) nib2[l] = nib[l] | nib[row_partner(l, step)];
            memcpy(nib, nib2, sizeof(nib));
        }
        uint32_t w[4];
        gsm::BC7Pack(blk[0], nib[0], w);
        gsm::BakeStoreBytes(out + (size_t)b * 16, w, 16u);
    }
}

// where the importer puts texel `lane` of destination record group 16 b: the byte offset of the block of splat i among the BC7 blocks, and the texel's
// row-major place inside it
uint64_t igh_bc7_block_of_splat(uint32_t i) { return gsm::BC7BlockOfSplat(i) * 16u; }
uint32_t igh_bc7_texel_of_lane(uint32_t lane) { return gsm::BC7TexelOfLane(lane); }

// rows[i] = the 45 raw SH floats of destination splat i: the points a Cluster* palette is computed from
void igh_sh_rows(const gsm::ImportSrc* in, uint32_t n, uint32_t linearize, uint32_t morton, float* rows) {
    float bounds[6];
    const std::vector<gsm::BakeRec> rec = ordered_records(*in, n, linearize, morton, bounds);
    for (uint32_t j = 0; j < n; ++j) memcpy(rows + (size_t)j * 45, rec[j].sh, 180);
}

// The whole import serially: the five blobs -- zero-filled by the caller, gs_import_blob_sizes bytes each; color_size = the colour blob's -- in the
// formats fmt (pos, scale, color, sh).  A Cluster* SH target takes the palette (means: k x 45, index: n, in destination order) the caller computed
// from igh_sh_rows' rows; else k = 0.  A BC7 colour target gets the tiles past the last chunk as the encoding of an all-zero block.
void igh_import(const gsm::ImportSrc* in, uint32_t n, const uint32_t* fmt, uint32_t linearize, uint32_t morton, const float* means, uint32_t k, const uint32_t* index,
                uint8_t* const* blobs, uint64_t color_size, float* bounds) {
    std::vector<gsm::BakeRec> rec = ordered_records(*in, n, linearize, morton, bounds);
    const gsm::BakeFormats f = { fmt[0], fmt[1], fmt[2], fmt[3], (fmt[0] | fmt[1] | fmt[2] | fmt[3]) != 0u ? 1u : 0u };
    for (uint32_t first = 0; first < n; first += 256u)
        gsm::BakeEncodeChunkSerial(rec.data() + first, std::min(256u, n - first), first, f, blobs[0], blobs[1], blobs[2], blobs[3], blobs[4], k ? index : nullptr);
    for (uint32_t j = 0; j < k; ++j) {
        uint32_t w[24];
        gsm::BakeEmitSHTableItem(means + (size_t)j * 45, w);
        gsm::BakeStoreBytes(blobs[3] + (size_t)j * 96, w, 96u);
    }
    if (fmt[2] != 3u) return;
    const float zero[16][4] = {};
    uint32_t w[4];
    gsm::BC7EncodeMode6(zero, w);
    for (uint64_t tile = (n + 255u) / 256u; tile < color_size / 256u; ++tile)
        for (uint32_t b = 0; b < 16u; ++b) gsm::BakeStoreBytes(blobs[2] + gsm::BC7BlockOfSplat((uint32_t)tile * 256u + b * 16u) * 16u, w, 16u);
}
}

#ifdef IMPORT_GPU_HARNESS_MAIN
#include <cstdio>
int main() {
    const uint32_t n = 257, K = 4096;                              // a one-splat last chunk
    std::vector<float> pos(n * 3), dc0(n * 3), sh(n * 45), opacity(n), scale(n * 3), rot(n * 4);
    uint32_t seed = 2468u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f) * 0.5f + 0.25f; };      // [0.25, 0.75): no zero, no NaN
    for (float* v : { pos.data(), dc0.data() }) for (uint32_t i = 0; i < n * 3; ++i) v[i] = rnd() * 4.0f - 2.0f;
    for (float& v : sh) v = rnd() - 0.5f;
    for (float* v : { opacity.data(), scale.data(), rot.data() }) for (uint32_t i = 0; i < n * (v == opacity.data() ? 1u : (v == scale.data() ? 3u : 4u)); ++i) v[i] = rnd();   // legal raw and linear
    const gsm::ImportSrc in = { pos.data(), dc0.data(), sh.data(), opacity.data(), scale.data(), rot.data() };
    int bad = 0;
    // the extremes of exp: the clamp at -87 / 88, far beyond, and 0
    const float xs[7] = { -1000.0f, -87.5f, -87.0f, 0.0f, 88.0f, 88.5f, 1000.0f };
    float es[7];
    igh_exp(xs, 7, es);
    bad += es[0] != es[2] || es[1] != es[2] || es[3] != 1.0f || es[4] != es[5] || es[5] != es[6] || !(es[2] > 0.0f) || !(es[4] < gsm::u2f(0x7f800000u));
    std::vector<float> lin((size_t)n * 11);
    std::vector<uint32_t> word(n);
    igh_linearize(&in, n, 1u, lin.data(), word.data());
    for (uint32_t i = 0; i < n; ++i) bad += !(lin[(size_t)i * 11 + 6] > 0.0f && lin[(size_t)i * 11 + 6] < 1.0f) || (word[i] >> 30) != (uint32_t)(lin[(size_t)i * 11 + 10] * 3.5f);
    // blocks: the all-zero one is 40 00 .. 00; one thread and sixteen lanes agree
    std::vector<float> texels((size_t)64 * 16 * 4, 0.0f);
    for (size_t i = 16 * 4; i < texels.size(); ++i) texels[i] = rnd() * 2.0f - 0.5f;
    std::vector<uint8_t> one(64 * 16), lanes(64 * 16);
    std::vector<uint32_t> flags(64);
    igh_bc7_blocks(texels.data(), 64, one.data(), flags.data());
    igh_bc7_blocks_lanes(texels.data(), 64, lanes.data());
    bad += one != lanes || one[0] != 0x40;
    for (int k = 1; k < 16; ++k) bad += one[k] != 0;
    // the whole import, every colour format and a Cluster4k table, the blobs at the importer's exact sizes
    const uint32_t targets[5][4] = { { 2, 3, 3, 8 }, { 2, 2, 2, 3 }, { 1, 1, 1, 2 }, { 0, 0, 0, 0 }, { 3, 0, 3, 1 } };
    const uint32_t vs[4] = { 12, 6, 4, 2 }, cs[4] = { 16, 8, 4, 1 }, ss[4] = { 192, 96, 60, 32 };
    std::vector<float> means((size_t)K * 45);
    for (float& m : means) m = rnd();
    std::vector<uint32_t> index(n);
    for (uint32_t j = 0; j < n; ++j) index[j] = (j * 2654435761u) % K;
    float bounds[6];
    for (const uint32_t* t : targets) {
        const bool chunked = (t[0] | t[1] | t[2] | t[3]) != 0u, clustered = t[3] > 3u;
        const size_t texels2 = (size_t)2048 * 16;
        std::vector<uint8_t> b0(((size_t)n * vs[t[0]] + 7) / 8 * 8, 0), b1(((size_t)n * (4 + vs[t[1]] + (clustered ? 2 : 0)) + 7) / 8 * 8, 0), b2(texels2 * cs[t[2]], 0),
            b3(clustered ? (size_t)K * 96 : (size_t)n * ss[t[3]], 0), b4(chunked ? (size_t)2 * 64 : 1, 0);
        uint8_t* blobs[5] = { b0.data(), b1.data(), b2.data(), b3.data(), b4.data() };
        for (uint32_t linearize = 0; linearize < 2u; ++linearize)
            igh_import(&in, n, t, linearize, 1u, means.data(), clustered ? K : 0u, index.data(), blobs, b2.size(), bounds);
        if (t[2] == 3u) for (size_t blk = 0; blk < b2.size() / 16; ++blk) bad += (b2[blk * 16] & 0x7f) != 0x40;      // every block is a mode-6 block
    }
    printf(bad ? "import gpu harness: %d mismatches\n" : "import gpu harness ok\n", bad);
    return bad != 0;
}
#endif
