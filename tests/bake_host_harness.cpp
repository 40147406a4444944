// Test-only: the bake's arithmetic (csrc/gs_device_math.h: LoadSplatDataFull, BakeLinearRecord, the chunk encode gsm::BakeEncodeChunkSerial, the Morton
// key gsm::BakeMortonCode) compiled for the HOST, so that tests/test_bake_model.py can hold it to the native importer (gs_import_encode, linearize = 0)
// byte for byte on a box without a GPU.  Never part of the shipped library.  With -DBAKE_HARNESS_MAIN it is a stand-alone program (its own main) that
// bakes a small all-fp32 asset it makes itself, 257 alive splats: the form a sanitizer build runs.
#include <algorithm>
#include <numeric>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
// codes[j] = the 63-bit Morton code of pos[j] inside bounds (min xyz, max xyz)
void bh_morton(const float* pos, uint32_t n, const float* bounds, uint64_t* codes) {
    for (uint32_t j = 0; j < n; ++j) codes[j] = gsm::BakeMortonCode({ pos[3 * j], pos[3 * j + 1], pos[3 * j + 2] }, bounds, bounds + 3);
}

// The splats src[0 .. n) of the asset (the alive ones, in index order) into the five blobs -- zero-filled by the caller, gs_import_blob_sizes bytes
// each -- in the formats fmt (pos, scale, color, sh); bounds: min xyz, max xyz of their positions.
void bh_bake(const gs_asset_desc* d, const uint32_t* src, uint32_t n, const uint32_t* fmt, uint32_t morton, uint8_t* const* blobs, float* bounds) {
    const gsm::AssetView a = gs::asset_view_of(*d);
    std::vector<gsm::BakeRec> rec(n);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = src[j], ci = i >> 8;
        gsm::SplatFull s;
        gsm::LoadSplatDataFull(a, i, ci, gsm::LoadSplatPosChunk(a, i, ci), s);
        gsm::BakeLinearRecord(s, rec[j]);
    }
    const float inf = gsm::u2f(0x7f800000u);
    for (int c = 0; c < 3; ++c) { bounds[c] = inf; bounds[3 + c] = -inf; }
    for (uint32_t j = 0; j < n; ++j) {
        const float p[3] = { rec[j].pos.x, rec[j].pos.y, rec[j].pos.z };
        for (int c = 0; c < 3; ++c) { bounds[c] = fminf(bounds[c], p[c]); bounds[3 + c] = fmaxf(bounds[3 + c], p[c]); }
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (morton) {
        std::vector<uint64_t> code(n);
        for (uint32_t j = 0; j < n; ++j) code[j] = gsm::BakeMortonCode(rec[j].pos, bounds, bounds + 3);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return code[x] < code[y]; });      // (code, rank)
    }
    const gsm::BakeFormats f = { fmt[0], fmt[1], fmt[2], fmt[3], (fmt[0] | fmt[1] | fmt[2] | fmt[3]) != 0u ? 1u : 0u };
    std::vector<gsm::BakeRec> chunk(256);
    for (uint32_t first = 0; first < n; first += 256u) {
        const uint32_t cnt = std::min(256u, n - first);
        for (uint32_t k = 0; k < cnt; ++k) chunk[k] = rec[order[first + k]];
        gsm::BakeEncodeChunkSerial(chunk.data(), cnt, first, f, blobs[0], blobs[1], blobs[2], blobs[3], blobs[4]);
    }
}
}

#ifdef BAKE_HARNESS_MAIN
#include <cstdio>
int main() {
    const uint32_t n = 300, aliveN = 257;
    const size_t texels = (size_t)2048 * 16;
    std::vector<float> pos(n * 3), color(texels * 4, 0.0f), sh(n * 48, 0.0f);
    std::vector<uint32_t> other(n * 4 + 4, 0u);
    uint32_t seed = 4321u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f) * 0.5f + 0.25f; };      // [0.25, 0.75): no zero, no NaN
    for (uint32_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) pos[i * 3 + c] = rnd();
        other[i * 4] = gsm::EncodeQuatToNorm10(gsm::PackSmallest3Rotation({ 0.1f, 0.2f, 0.3f, 0.9f }));
        for (int c = 0; c < 3; ++c) other[i * 4 + 1 + c] = gsm::f2u(rnd());
        uint32_t px, py;
        gsm::SplatIndexToPixelIndex(i, px, py);
        for (int c = 0; c < 4; ++c) color[((size_t)py * 2048 + px) * 4 + c] = rnd();
        for (int c = 0; c < 45; ++c) sh[i * 48 + c] = rnd();
    }
    gs_asset_desc d;
    memset(&d, 0, sizeof(d));
    d.splat_count = n;
    d.pos_data = pos.data(); d.pos_size = pos.size() * 4;
    d.other_data = other.data(); d.other_size = (uint64_t)n * 16;
    d.color_data = color.data(); d.color_size = color.size() * 4;
    d.sh_data = sh.data(); d.sh_size = sh.size() * 4;
    std::vector<uint32_t> src;
    for (uint32_t i = 0; i < n && src.size() < aliveN; ++i) if (i % 7u != 3u) src.push_back(i);       // 257 alive: a one-splat last chunk
    int bad = src.size() != aliveN;
    float bounds[6];
    // every format once, the blobs at the exact sizes of the importer so that a write past an end is caught
    const uint32_t targets[5][4] = { { 2, 2, 2, 3 }, { 1, 1, 1, 2 }, { 3, 3, 2, 1 }, { 0, 0, 0, 0 }, { 0, 3, 0, 0 } };
    const uint32_t vs[4] = { 12, 6, 4, 2 }, cs[3] = { 16, 8, 4 }, ss[4] = { 192, 96, 60, 32 };
    for (const uint32_t* t : targets) {
        const bool chunked = (t[0] | t[1] | t[2] | t[3]) != 0u;
        std::vector<uint8_t> b0(((size_t)aliveN * vs[t[0]] + 7) / 8 * 8, 0), b1(((size_t)aliveN * (4 + vs[t[1]]) + 7) / 8 * 8, 0), b2(texels * cs[t[2]], 0),
            b3((size_t)aliveN * ss[t[3]], 0), b4(chunked ? (size_t)2 * 64 : 1, 0);
        uint8_t* blobs[5] = { b0.data(), b1.data(), b2.data(), b3.data(), b4.data() };
        bh_bake(&d, src.data(), aliveN, t, 1u, blobs, bounds);
        if (!chunked) {                                            // the identity's known answer, through the Morton order: every source position is there once
            std::vector<float> got((float*)b0.data(), (float*)b0.data() + aliveN * 3), want;
            for (uint32_t i : src) want.insert(want.end(), { pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] });
            auto key = [](std::vector<float>& v) { std::vector<std::vector<float>> r; for (size_t k = 0; k < v.size(); k += 3) r.push_back({ v[k], v[k + 1], v[k + 2] }); std::sort(r.begin(), r.end()); return r; };
            bad += key(got) != key(want);
        }
    }
    printf(bad ? "bake harness: %d mismatches\n" : "bake harness ok\n", bad);
    return bad != 0;
}
#endif
