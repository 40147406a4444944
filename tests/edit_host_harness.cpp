// Test-only: the edit kernels' per-splat arithmetic (csrc/gs_device_math.h: IsSplatCut, EditSelectionHit, EditSplatBounds) compiled for the
// HOST, so that tests/test_edit_model.py can hold it to tests/edit_model.py bit for bit on a box without a GPU.  Never part of the shipped library.
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
// hit[i], cut[i]: 0 / 1; lo[i * 3 + k], hi[i * 3 + k]: the sortable bounds of splat i
void eh_eval(const gs_asset_desc* d, const gs_frame_params* p, const float rect[4], const gs_cutout* cutouts, uint32_t cutoutCount,
             uint8_t* hit, uint8_t* cut, uint32_t* lo, uint32_t* hi) {
    const gsm::AssetView a = gs::asset_view_of(*d);
    gsm::EditView e; e.deletedBits = nullptr; e.cutouts = (const uint32_t*)cutouts; e.cutoutCount = cutoutCount;
    const gsm::EditSelect S = gs::edit_select_of(*p, rect);
    for (uint32_t i = 0; i < a.n; ++i) {
        const gsm::V3 pos = gsm::LoadSplatPosChunk(a, i, i >> 8);      // (the kernels pass blockIdx.x)
        hit[i] = gsm::EditSelectionHit(S, e, pos) ? 1 : 0;
        cut[i] = gsm::IsSplatCut(e, pos.x, pos.y, pos.z) ? 1 : 0;
        gsm::EditSplatBounds(pos, lo + (size_t)i * 3, hi + (size_t)i * 3);
    }
}
}
