// Test-only: what a bake to a Cluster* SH target adds to the arithmetic of csrc/gs_device_math.h -- the SH rows the palette is computed from, the `other`
// record with its u16 table index (gsm::BakeEmitOther: 8, 10, 12 or 18 bytes), the table item (gsm::BakeEmitSHTableItem) and the chunk encode that
// writes no SH item (gsm::BakeEncodeChunkSerial with shIndex) -- compiled for the HOST, so that tests/test_bake_cluster_model.py can hold it to the
// native importer's bytes on a box without a GPU.  Never part of the shipped library.  With -DBAKE_CLUSTER_HARNESS_MAIN it is a stand-alone program
// (its own main) over a small all-fp32 asset it makes itself, 257 alive splats: the form a sanitizer build runs.
#include <algorithm>
#include <numeric>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

namespace {

// the linear records of the splats src[0 .. n) in destination order (Morton order of their positions when asked for), and the position bounds
std::vector<gsm::BakeRec> ordered_records(const gs_asset_desc* d, const uint32_t* src, uint32_t n, uint32_t morton, float* bounds) {
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
    if (!morton) return rec;
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::vector<uint64_t> code(n);
    for (uint32_t j = 0; j < n; ++j) code[j] = gsm::BakeMortonCode(rec[j].pos, bounds, bounds + 3);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return code[x] < code[y]; });      // (code, rank)
    std::vector<gsm::BakeRec> out(n);
    for (uint32_t j = 0; j < n; ++j) out[j] = rec[order[j]];
    return out;
}

} // namespace

extern "C" {
// rows[i] = the 45 raw SH floats of destination splat i: the points the palette is computed from
void bch_sh_rows(const gs_asset_desc* d, const uint32_t* src, uint32_t n, uint32_t morton, float* rows) {
    float bounds[6];
    const std::vector<gsm::BakeRec> rec = ordered_records(d, src, n, morton, bounds);
    for (uint32_t j = 0; j < n; ++j) memcpy(rows + (size_t)j * 45, rec[j].sh, 180);
}

// The splats src[0 .. n) into the five blobs of a Cluster* SH target -- zero-filled by the caller, gs_import_blob_sizes bytes each -- with the palette
// (means: k x 45, index: n, in destination order) the caller computed from bch_sh_rows' rows.  fmt: pos, scale, color, sh
void bch_bake(const gs_asset_desc* d, const uint32_t* src, uint32_t n, const uint32_t* fmt, uint32_t morton, const float* means, uint32_t k, const uint32_t* index,
              uint8_t* const* blobs, float* bounds) {
    std::vector<gsm::BakeRec> rec = ordered_records(d, src, n, morton, bounds);
    const gsm::BakeFormats f = { fmt[0], fmt[1], fmt[2], fmt[3], 1u };      // every Cluster* target is chunked
    for (uint32_t first = 0; first < n; first += 256u)
        gsm::BakeEncodeChunkSerial(rec.data() + first, std::min(256u, n - first), first, f, blobs[0], blobs[1], blobs[2], blobs[3], blobs[4], index);
    for (uint32_t j = 0; j < k; ++j) {
        uint32_t w[24];
        gsm::BakeEmitSHTableItem(means + (size_t)j * 45, w);
        gsm::BakeStoreBytes(blobs[3] + (size_t)j * 96, w, 96u);
    }
}

// one `other` record on its own: returns its size in bytes; out: 20 bytes
uint32_t bch_other(uint32_t rot, const float* scale, uint32_t scaleFmt, uint32_t clustered, uint32_t index, uint8_t* out) {
    uint32_t w[5];
    const uint32_t bytes = gsm::BakeEmitOther(rot, { scale[0], scale[1], scale[2] }, scaleFmt, clustered != 0u, index, w);
    gsm::BakeStoreBytes(out, w, 20u);
    return bytes;
}
}

#ifdef BAKE_CLUSTER_HARNESS_MAIN
#include <cstdio>
int main() {
    const uint32_t n = 300, aliveN = 257, K = 4096;
    const size_t texels = (size_t)2048 * 16;
    std::vector<float> pos(n * 3), color(texels * 4, 0.0f), sh(n * 48, 0.0f);
    std::vector<uint32_t> other(n * 4 + 4, 0u);
    uint32_t seed = 9876u;
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
    // the rows, without the Morton order, are the source's SH floats
    std::vector<float> rows((size_t)aliveN * 45);
    bch_sh_rows(&d, src.data(), aliveN, 0u, rows.data());
    for (uint32_t j = 0; j < aliveN; ++j) bad += memcmp(&rows[(size_t)j * 45], &sh[(size_t)src[j] * 48], 180) != 0;
    // a palette of the right shape (the values are beside the point here): K means, an index per splat that uses both bytes of the halfword
    std::vector<float> means((size_t)K * 45);
    for (float& m : means) m = rnd();
    std::vector<uint32_t> index(aliveN);
    for (uint32_t j = 0; j < aliveN; ++j) index[j] = (j * 2654435761u) % K;
    float bounds[6];
    const uint32_t vs[4] = { 12, 6, 4, 2 };
    for (uint32_t scaleFmt = 0; scaleFmt < 4; ++scaleFmt) {                   // 18-, 12-, 10- and 8-byte `other` records, the blobs at the importer's exact sizes
        const uint32_t t[4] = { 2, scaleFmt, 2, 8 }, othSz = 4 + vs[scaleFmt] + 2;
        std::vector<uint8_t> b0(((size_t)aliveN * 4 + 7) / 8 * 8, 0), b1(((size_t)aliveN * othSz + 7) / 8 * 8, 0), b2(texels * 4, 0), b3((size_t)K * 96, 0), b4((size_t)2 * 64, 0);
        uint8_t* blobs[5] = { b0.data(), b1.data(), b2.data(), b3.data(), b4.data() };
        bch_bake(&d, src.data(), aliveN, t, 0u, means.data(), K, index.data(), blobs, bounds);
        for (uint32_t j = 0; j < aliveN; ++j) {
            uint16_t got;
            memcpy(&got, &b1[(size_t)j * othSz + 4 + vs[scaleFmt]], 2);
            bad += got != (uint16_t)index[j];
        }
        for (uint32_t j = 0; j < K; ++j) {
            uint16_t h[48];
            memcpy(h, &b3[(size_t)j * 96], 96);
            bad += (h[45] | h[46] | h[47]) != 0;
            for (int c = 0; c < 45; ++c) bad += h[c] != (uint16_t)gsm::f32tof16(means[(size_t)j * 45 + c]);
        }
    }
    printf(bad ? "bake cluster harness: %d mismatches\n" : "bake cluster harness ok\n", bad);
    return bad != 0;
}
#endif
