// Test-only: the SPZ export's packer (csrc/gs_device_math.h: gsm::SpzPack*, SpzCode8, SpzAutoFractBits) and the host side of its argument checks
// (csrc/gs_params.h: spz_params_refusal, spz_alive_refusal, spz_body_bytes) compiled for the HOST, so that tests/test_spz_export_model.py can hold them
// to tests/spz_export_model.py byte for byte on a box without a GPU.  Never part of the shipped library.  With -DSPZ_EXPORT_HARNESS_MAIN it is a
// stand-alone program (its own main) that packs records it makes itself -- every special value in every column, every SH level, buffers at their exact
// sizes on the heap -- for a run under the host sanitizers.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
void sxh_code8(const float* t, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)gsm::SpzCode8(t[i]);
}

// out: the 24-bit codes
void sxh_coordinates(const float* p, uint64_t n, uint32_t fractBits, uint32_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = gsm::SpzPackCoordinate(p[i], fractBits);
}

// q: n x (w, x, y, z) as the export record holds them; out: n x 3 bytes
void sxh_rotations(const float* q, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; ++i) gsm::SpzPackRotation(q[i * 4], q[i * 4 + 1], q[i * 4 + 2], q[i * 4 + 3], out + i * 3);
}

uint32_t sxh_auto_fract_bits(const float* bounds6) { return gsm::SpzAutoFractBits(bounds6); }

uint64_t sxh_body_bytes(uint64_t n, uint32_t shLevel) { return gs::spz_body_bytes(n, shLevel); }

// 0 = acceptable
int32_t sxh_params_refused(const gs_spz_params* s) { return gs::spz_params_refusal(*s) ? 1 : 0; }
int32_t sxh_alive_refused(uint64_t alive) { return gs::spz_alive_refusal(alive) ? 1 : 0; }

// The body of n splats as the library lays it out: rec = n x 62 floats (ExportSplatLinear's records), opacity = n decoded linear opacities; out =
// spz_body_bytes(n, shLevel) bytes.  Splat by splat through gsm::SpzPackSplat, each column at its place in the file
void sxh_body(const float* rec, const float* opacity, uint32_t n, uint32_t shLevel, uint32_t fractBits, uint8_t* out) {
    const uint32_t k = gsm::SpzShCoeffs(shLevel);
    uint32_t head[4];
    gsm::SpzHeaderWords(n, shLevel, fractBits, head);
    memcpy(out, head, 16);
    uint8_t* col[gsm::kSpzColumns];
    uint64_t at = 16;
    for (uint32_t c = 0; c < gsm::kSpzColumns; ++c) { col[c] = out + at; at += (uint64_t)n * gsm::SpzColumnWidth(c, k); }
    for (uint64_t i = 0; i < n; ++i)
        gsm::SpzPackSplat(rec + i * 62, opacity[i], fractBits, k, col[0] + i * 9, col[1] + i, col[2] + i * 3, col[3] + i * 3, col[4] + i * 3, col[5] + i * 3 * k);
}
}

#ifdef SPZ_EXPORT_HARNESS_MAIN
int main() {
    const float inf = INFINITY, nan = NAN;
    const float special[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1.5f, 2.5f, 254.5f, 255.5f, 8388607.5f, -8388608.5f, 1.0e30f, -1.0e30f, inf, -inf, nan, 1.0e-45f, 3.4028235e38f };
    const uint32_t m = sizeof(special) / sizeof(special[0]);
    for (uint32_t level = 0; level <= 3; ++level) {
        for (uint32_t fract : { 0u, 1u, 12u, 24u }) {
            const uint32_t n = m * 3u + 1u;
            std::vector<float> rec((size_t)n * 62), op(n);
            for (uint32_t i = 0; i < n; ++i) {
                for (uint32_t k = 0; k < 62; ++k) rec[(size_t)i * 62 + k] = special[(i + k * 7u) % m] * (float)(1u + i / m);
                op[i] = special[i % m];
            }
            const uint64_t bytes = gs::spz_body_bytes(n, level);
            uint8_t* body = (uint8_t*)malloc(bytes);               // at its exact size: a byte past any column is a report
            sxh_body(rec.data(), op.data(), n, level, fract, body);
            if (body[0] != 'N' || body[3] != 'P' || body[12] != level || body[13] != fract) { printf("bad header\n"); return 1; }
            free(body);
        }
    }
    std::vector<uint8_t> codes(m);
    sxh_code8(special, m, codes.data());
    std::vector<uint32_t> fixed(m);
    for (uint32_t f = 0; f <= 24; ++f) sxh_coordinates(special, m, f, fixed.data());
    float bounds[6] = { -inf, nan, -3.0f, 2047.9f, inf, 0.0f };
    (void)sxh_auto_fract_bits(bounds);
    gs_spz_params s = { 3u, GS_SPZ_FRACT_AUTO, -1, 0u };
    if (sxh_params_refused(&s) || !sxh_alive_refused(0) || sxh_alive_refused(1)) { printf("bad checks\n"); return 1; }
    printf("spz export harness ok\n");
    return 0;
}
#endif
