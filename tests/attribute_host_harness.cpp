// Test-only: the attribute tools' arithmetic (csrc/gs_device_math.h: gsm::AttributeValue over the partial decodes LoadSplatScale / LoadSplatOpacity /
// LoadSplatBaseColor, AttributeInRange, AttributeBin, FloatToSortableUint and its inverse) compiled for the HOST and run per splat the way the kernels
// of gs_attributes.hip run it, so that tests/test_attribute_host.py can hold it to tests/attribute_model.py bit for bit on a box without a GPU.  Never
// part of the shipped library.
// A stand-alone program (its own main):  attribute_host_harness <in> <out>
//   in : u32 n, posFmt, scaleFmt, colorFmt, shFmt, chunkCount, attr, bins; f32 q[3], lo, hi, s; u64 bytes[5]; the blobs pos, other, color, sh, chunk
//   out: n x { u32 value bits, u32 KEY, u32 histogram word (0 when bins == 0), u32 lo <= v <= hi }
// Without arguments it runs the same code over an input it makes itself and checks what needs no model: the form a sanitizer build runs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_device_math.h"

struct Out { uint32_t value, key, bin, in; };

static std::vector<Out> run(const gsm::AssetView& a, int attr, gsm::V3 q, float lo, float hi, float s, uint32_t bins) {
    std::vector<Out> out(a.n);
    for (uint32_t i = 0; i < a.n; ++i) {
        const uint32_t ci = i >> 8;
        const float v = gsm::AttributeValue(a, attr, i, ci, gsm::LoadSplatPosChunk(a, i, ci), q);
        out[i] = { gsm::f2u(v), gsm::FloatToSortableUint(v), bins ? gsm::AttributeBin(v, lo, hi, s, bins) : 0u, gsm::AttributeInRange(v, lo, hi) ? 1u : 0u };
    }
    return out;
}

static int self_test() {
    // six fp32 chunk-less splats: an ordinary one, a NaN scale beside numbers, -0 / +0 scales, an overflowing product, opacities on lo, hi and outside
    const uint32_t n = 6;
    const float nan = gsm::u2f(0x7fc00000u), inf = gsm::u2f(0x7f800000u);
    std::vector<float> pos = { 1, 2, 3, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const float scale[n][3] = { { 0.1f, 0.7f, 0.3f }, { nan, 2.0f, nan }, { -0.0f, 0.0f, -0.0f }, { 3e38f, 3e38f, 1.0f }, { 1, 1, 1 }, { 1, 1, 1 } };
    const float opacity[n] = { 0.6f, 0.125f, 0.875f, 0.1f, 0.9f, nan };
    std::vector<uint32_t> other(n * 4 + 4, 0u);
    std::vector<float> texels(2048 * 16 * 4 + 4, 0.0f);
    for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) other[i * 4 + 1 + k] = gsm::f2u(scale[i][k]);
        uint32_t x, y;
        gsm::SplatIndexToPixelIndex(i, x, y);
        float* t = &texels[((size_t)y * 2048 + x) * 4];
        t[0] = 0.25f; t[1] = 0.5f; t[2] = 1.0f; t[3] = opacity[i];
    }
    pos.resize(pos.size() + 4);
    gsm::AssetView a = {};
    a.pos = (const uint8_t*)pos.data(); a.other = (const uint8_t*)other.data(); a.color = (const uint8_t*)texels.data(); a.sh = nullptr; a.chunk = nullptr;
    a.n = n;
    const gsm::V3 q = { 0, 0, 0 };
    bool ok = true;
    const std::vector<Out> mx = run(a, gsm::kAttrScaleMax, q, 0, 1, 1, 0), mn = run(a, gsm::kAttrScaleMin, q, 0, 1, 1, 0), vol = run(a, gsm::kAttrVolume, q, 0, 1, 1, 0);
    ok = ok && mx[0].value == gsm::f2u(0.7f) && mn[0].value == gsm::f2u(0.1f) && mx[1].value == gsm::f2u(2.0f) && mn[1].value == gsm::f2u(2.0f);
    ok = ok && mx[2].value == 0x80000000u && mn[2].value == 0x80000000u;                       // the first operand of a +-0 tie
    ok = ok && vol[3].value == gsm::f2u(inf) && (vol[1].value & 0x7fffffffu) > 0x7f800000u;   // an overflow; a NaN
    const float lo = 0.125f, hi = 0.875f, s = 4.0f / (hi - lo);
    const std::vector<Out> op = run(a, gsm::kAttrOpacity, q, lo, hi, s, 4);
    ok = ok && op[0].bin == 2u && op[1].bin == 0u && op[2].bin == 3u && op[3].bin == 4u && op[4].bin == 5u && op[5].bin == 6u;
    ok = ok && op[1].in == 1u && op[2].in == 1u && op[3].in == 0u && op[4].in == 0u && op[5].in == 0u;
    const std::vector<Out> d2 = run(a, gsm::kAttrDist2, q, 0, 1, 1, 0), luma = run(a, gsm::kAttrLuma, q, 0, 1, 1, 0);
    ok = ok && d2[0].value == gsm::f2u(14.0f) && luma[0].value == gsm::f2u((0.299f * 0.25f + 0.587f * 0.5f) + 0.114f * 1.0f);
    ok = ok && gsm::FloatToSortableUint(-0.0f) + 1u == gsm::FloatToSortableUint(0.0f);
    for (const Out& o : op) ok = ok && gsm::f2u(gsm::SortableUintToFloat(o.key)) == o.value;
    if (!ok) { fprintf(stderr, "attribute_host_harness: self test failed\n"); return 1; }
    printf("attribute_host_harness ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc != 3) { fprintf(stderr, "usage: %s [<in> <out>]\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t h[8];
    float f[6];
    uint64_t bytes[5];
    bool ok = fread(h, 4, 8, in) == 8 && fread(f, 4, 6, in) == 6 && fread(bytes, 8, 5, in) == 5;
    std::vector<uint8_t> blob[5];
    for (int k = 0; ok && k < 5; ++k) {
        blob[k].assign((size_t)bytes[k] + 16, 0);                  // the dword stitching of LoadUInt may touch the dword after the last record
        ok = bytes[k] == 0 || fread(blob[k].data(), 1, (size_t)bytes[k], in) == (size_t)bytes[k];
    }
    fclose(in);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    gsm::AssetView a = {};
    a.pos = blob[0].data(); a.other = blob[1].data(); a.color = blob[2].data(); a.sh = blob[3].data(); a.chunk = blob[4].data();
    a.n = h[0]; a.posFmt = h[1]; a.scaleFmt = h[2]; a.colorFmt = h[3]; a.shFmt = h[4]; a.chunkCount = h[5];
    const std::vector<Out> out = run(a, (int)h[6], { f[0], f[1], f[2] }, f[3], f[4], f[5], h[7]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = a.n == 0 || fwrite(out.data(), sizeof(Out), a.n, o) == a.n;
    if (fclose(o) != 0 || !ok) { fprintf(stderr, "short output\n"); return 2; }
    return 0;
}
