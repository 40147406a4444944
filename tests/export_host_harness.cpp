// Test-only: the export's per-splat arithmetic (csrc/gs_device_math.h: LogDetFull, CalcSHRot, LoadSplatDataFull, ExportSplat) compiled for the
// HOST, so that tests/test_export_model.py can hold it to tests/export_model.py bit for bit on a box without a GPU.  Never part of the shipped library.
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
void xh_logdet(const float* x, float* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = gsm::LogDetFull(x[i]);
}

// out: sh1 (9), sh2 (25), sh3 (49) floats, rows first
void xh_bands(const float* o2w, float* out) {
    gsm::SHRot R;
    gsm::CalcSHRot(o2w, R);
    memcpy(out, &R, sizeof(R));
}

uint32_t xh_sizes(uint32_t which) { return which == 0 ? (uint32_t)sizeof(gsm::SHRot) : (which == 1 ? (uint32_t)sizeof(gs_export_params) : (uint32_t)sizeof(gsm::ExportXform)); }

// out: n x 62 floats, what export_records_kernel leaves in reference-shaped mode
void xh_export(const gs_asset_desc* d, const gs_export_params* p, const gs_cutout* cutouts, uint32_t cutoutCount, float* out) {
    const gsm::AssetView a = gs::asset_view_of(*d);
    gsm::EditView e; e.deletedBits = nullptr; e.cutouts = (const uint32_t*)cutouts; e.cutoutCount = cutoutCount;
    const gsm::ExportXform X = gs::export_xform_of(*p);
    for (uint32_t i = 0; i < a.n; ++i) {
        const gsm::V3 pos = gsm::LoadSplatPosChunk(a, i, i >> 8);      // (the kernels pass the workgroup's chunk)
        const bool cut = gsm::IsSplatCut(e, pos.x, pos.y, pos.z);
        gsm::ExportSplat(a, X, i, i >> 8, pos, cut, out + (size_t)i * 62);
    }
}
}
