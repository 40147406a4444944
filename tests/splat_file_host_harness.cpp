// Test-only: the two file sources of the GPU import (csrc/gs_device_math.h: gsm::PlyRowRecord / gsm::PlyRowPosition over a PLY's vertex rows as they
// lie in the file, gsm::SpzRecord / gsm::SpzPosition over an SPZ's gunzipped stream) compiled for the HOST, next to gsm::ImportRecord over six arrays,
// so that tests/test_splat_file_model.py can hold them to the arrays of gs_ply_open / gs_spz_open bit for bit on a box without a GPU.  Never part of
// the shipped library.  With -DSPLAT_FILE_HARNESS_MAIN it is a stand-alone program (its own main) over inputs it makes itself, every buffer at its
// exact size: the form a sanitizer build runs.
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
uint32_t sfh_record_bytes() { return (uint32_t)sizeof(gsm::BakeRec); }

void sfh_import_records(const gsm::ImportSrc* in, uint32_t n, uint32_t linearize, gsm::BakeRec* out) {
    for (uint32_t i = 0; i < n; ++i) gsm::ImportRecord(*in, i, linearize, out[i]);
}

// off: the 62 offsets of gs_splat_file_info; pos[n][3] = PlyRowPosition.  path: 2 = the loads gsm::PlyRowLayout chooses, 1 = no merged loads of the
// INRIA layout, 0 = byte loads; returns the layout's flags, aligned | inria << 1
uint32_t sfh_ply_records(const uint8_t* rows, uint32_t stride, const int32_t* off, uint32_t path, uint32_t n, gsm::BakeRec* out, float* pos) {
    gsm::PlyRowSrc s;
    s.rows = rows; s.stride = stride;
    for (int k = 0; k < gsm::kPlyOffsets; ++k) s.off[k] = off[k];
    gsm::PlyRowLayout(s);
    const uint32_t flags = s.aligned | (s.inria << 1);
    if (path < 2u) s.inria = 0u;
    if (path < 1u) s.aligned = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        gsm::PlyRowRecord(s, i, out[i]);
        const gsm::V3 p = gsm::PlyRowPosition(s, i);
        pos[i * 3] = p.x; pos[i * 3 + 1] = p.y; pos[i * 3 + 2] = p.z;
    }
    return flags;
}

void sfh_spz_records(const uint8_t* stream, uint32_t n, uint32_t shCoeffs, uint32_t fractBits, gsm::BakeRec* out, float* pos) {
    const gsm::SpzSrc s = { stream, n, shCoeffs, fractBits };
    for (uint32_t i = 0; i < n; ++i) {
        gsm::SpzRecord(s, i, out[i]);
        const gsm::V3 p = gsm::SpzPosition(s, i);
        pos[i * 3] = p.x; pos[i * 3 + 1] = p.y; pos[i * 3 + 2] = p.z;
    }
}
}

#ifdef SPLAT_FILE_HARNESS_MAIN
#include <cstdio>
int main() {
    uint32_t seed = 97531u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    int bad = 0;
    const uint32_t n = 67;
    // PLY rows in the INRIA order (stride 248: the merged loads, or with the f_rest properties absent the table's dword loads), and behind one foreign
    // byte (stride 249: byte loads)
    for (uint32_t lead = 0; lead < 2u; ++lead) {
        for (uint32_t rest = 0; rest < 2u; ++rest) {
            const uint32_t floats = rest ? 59u : 14u, stride = lead + 62u * 4u;
            std::vector<uint8_t> rows((size_t)n * stride);                    // exactly the rows: a read past the last one is the sanitizer's
            std::vector<float> pos(n * 3), dc0(n * 3), sh(n * 45, 0.0f), opacity(n), scale(n * 3), rot(n * 4);
            int32_t off[gsm::kPlyOffsets];
            for (int k = 0; k < gsm::kPlyOffsets; ++k) off[k] = k < (int)floats ? (int32_t)(lead + 4u * (uint32_t)gsm::PlyInriaFloat(k)) : -1;
            for (uint32_t i = 0; i < n; ++i) {
                for (uint32_t k = 0; k < floats; ++k) {
                    const float v = (float)(rnd() & 0xffffu) * (1.0f / 65536.0f) + 0.25f;
                    memcpy(&rows[(size_t)i * stride + (uint32_t)off[k]], &v, 4);
                    if (k < 3u) pos[i * 3 + k] = v;
                    else if (k < 6u) dc0[i * 3 + k - 3u] = v;
                    else if (k == 6u) opacity[i] = v;
                    else if (k < 10u) scale[i * 3 + k - 7u] = v;
                    else if (k < 14u) rot[i * 4 + k - 10u] = v;
                    else { const uint32_t r = k - 14u; sh[i * 45 + (r % 15u) * 3u + r / 15u] = v; }      // ReorderSHs
                }
            }
            const gsm::ImportSrc in = { pos.data(), dc0.data(), sh.data(), opacity.data(), scale.data(), rot.data() };
            std::vector<gsm::BakeRec> want(n), got(n);
            std::vector<float> p(n * 3);
            sfh_import_records(&in, n, 1u, want.data());
            for (uint32_t path = 0; path < 3u; ++path) {
                bad += sfh_ply_records(rows.data(), stride, off, path, n, got.data(), p.data()) != (lead ? 0u : (rest ? 3u : 1u));
                bad += memcmp(got.data(), want.data(), (size_t)n * sizeof(gsm::BakeRec)) != 0;
                bad += memcmp(p.data(), pos.data(), (size_t)n * 12) != 0;
            }
        }
    }
    // SPZ streams of every SH level, exactly as long as their columns: the fifteen-coefficient read of the last points leaves the SH array
    for (uint32_t level = 0; level < 4u; ++level) {
        const uint32_t coeffs = level == 1u ? 3u : (level == 2u ? 8u : (level == 3u ? 15u : 0u));
        std::vector<uint8_t> stream(16u + (size_t)n * (9u + 1u + 9u + 3u * coeffs));
        for (size_t k = 16; k < stream.size(); ++k) stream[k] = (uint8_t)rnd();
        std::vector<gsm::BakeRec> got(n);
        std::vector<float> p(n * 3);
        sfh_spz_records(stream.data(), n, coeffs, 8u * level, got.data(), p.data());
        for (uint32_t i = 0; i < n; ++i) {
            bad += memcmp(&got[i].pos, &p[i * 3], 12) != 0 || !(got[i].scale.x > 0.0f) || !(got[i].col.w >= 0.0f && got[i].col.w <= 1.0f);
            for (uint32_t k = coeffs * 3u; k < 45u && i == n - 1u; ++k) bad += got[i].sh[k] != 0.0f;      // past the array: 128 = 0
        }
    }
    printf(bad ? "splat file harness: %d mismatches\n" : "splat file harness ok\n", bad);
    return bad != 0;
}
#endif
