// Test-only: the edit kernels' per-splat arithmetic (csrc/gs_device_math.h: IsSplatCut, EditSelectionHit, EditSplatBounds) compiled for the
// HOST, so that tests/test_edit_model.py can hold it to tests/edit_model.py bit for bit on a box without a GPU.  Never part of the shipped library.
#include "../include/gsplat_c.h"
#include "../unitygaussiansplatting_amd/csrc/gs_device_math.h"

extern "C" {
// hit[i], cut[i]: 0 / 1; lo[i * 3 + k], hi[i * 3 + k]: the sortable bounds of splat i
void eh_eval(const gs_asset_desc* d, const gs_frame_params* p, const float rect[4], const gs_cutout* cutouts, uint32_t cutoutCount,
             uint8_t* hit, uint8_t* cut, uint32_t* lo, uint32_t* hi) {
    gsm::AssetView a;
    a.pos = (const uint8_t*)d->pos_data; a.other = (const uint8_t*)d->other_data; a.color = (const uint8_t*)d->color_data;
    a.sh = (const uint8_t*)d->sh_data; a.chunk = (const uint8_t*)d->chunk_data;
    a.n = d->splat_count; a.posFmt = d->pos_format; a.scaleFmt = d->scale_format; a.colorFmt = d->color_format; a.shFmt = d->sh_format;
    a.chunkCount = (d->chunk_data && d->chunk_size) ? (uint32_t)(d->chunk_size / 64) : 0;
    gsm::EditView e; e.deletedBits = nullptr; e.cutouts = (const uint32_t*)cutouts; e.cutoutCount = cutoutCount;
    gsm::EditSelect S;
    memcpy(S.o2w, p->matrix_object_to_world, sizeof(S.o2w));
    memcpy(S.vp, p->matrix_vp, sizeof(S.vp));
    S.screenW = p->screen_w; S.screenH = p->screen_h;
    memcpy(S.rect, rect, sizeof(S.rect));
    for (uint32_t i = 0; i < a.n; ++i) {
        const gsm::V3 pos = gsm::LoadSplatPosChunk(a, i, i >> 8);      // (the kernels pass blockIdx.x)
        hit[i] = gsm::EditSelectionHit(S, e, pos) ? 1 : 0;
        cut[i] = gsm::IsSplatCut(e, pos.x, pos.y, pos.z) ? 1 : 0;
        gsm::EditSplatBounds(pos, lo + (size_t)i * 3, hi + (size_t)i * 3);
    }
}
}
