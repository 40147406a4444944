// gs_params.h -- the C ABI's structs (include/gsplat_c.h) turned into the kernels' arguments (gs_device_math.h), once.  The .hip files call these,
// and so do the host harnesses of the CPU model tests (tests/*_harness.cpp, tests/copy_kernel_host_emulation.cpp): what those tests exercise are
// the lines the library ships.  No HIP header: plain g++ -std=c++17 compiles it.
#pragma once
#include <string.h>

#include "../../include/gsplat_c.h"
#include "gs_device_math.h"

namespace gs {

// the descriptor's formats, counts and pointers (gs_asset_create replaces the five pointers by its device blobs)
inline gsm::AssetView asset_view_of(const gs_asset_desc& d) {
    gsm::AssetView a;
    a.pos = (const uint8_t*)d.pos_data; a.other = (const uint8_t*)d.other_data; a.color = (const uint8_t*)d.color_data;
    a.sh = (const uint8_t*)d.sh_data; a.chunk = (const uint8_t*)d.chunk_data;
    a.n = d.splat_count; a.posFmt = d.pos_format; a.scaleFmt = d.scale_format; a.colorFmt = d.color_format; a.shFmt = d.sh_format;
    a.chunkCount = (d.chunk_data && d.chunk_size) ? (uint32_t)(d.chunk_size / 64) : 0;
    return a;
}

// null: the exact identity
inline gsm::CopyXform copy_xform_of(const gs_copy_params* p) {
    static const gs_copy_params kIdentity = { { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 }, { 0, 0, 0, 1 }, { 1, 1, 1 } };
    if (!p) p = &kIdentity;
    gsm::CopyXform X;
    memcpy(X.m, p->matrix, sizeof(X.m));
    memcpy(X.rot, p->rotation, sizeof(X.rot));
    memcpy(X.scale, p->scale, sizeof(X.scale));
    gsm::CalcSHRot(p->matrix, X.sh);                               // once per call, not once per thread
    return X;
}

inline gsm::ExportXform export_xform_of(const gs_export_params& p) {
    gsm::ExportXform X;
    memset(&X, 0, sizeof(X));
    X.bake = p.bake_transform ? 1u : 0u;
    memcpy(X.o2w, p.matrix_object_to_world, sizeof(X.o2w));
    memcpy(X.rot, p.rotation, sizeof(X.rot));
    memcpy(X.scale, p.scale, sizeof(X.scale));
    if (X.bake) gsm::CalcSHRot(p.matrix_object_to_world, X.sh);    // once per call, not once per thread
    return X;
}

// The SPZ export's argument checks, host logic alone (so a host harness holds them without a device).  Each returns what is wrong, or null.
// spz_params_refusal: before anything is launched; spz_alive_refusal: once the alive count is known -- a file the readers refuse is not written
constexpr uint32_t kSpzSliceDefault = 64u << 20, kSpzSliceMin = 4096u;
inline const char* spz_params_refusal(const gs_spz_params& s) {
    if (s.sh_level > 3u) return "export: sh_level must be 0..3";
    if (s.fract_bits > 24u && s.fract_bits != GS_SPZ_FRACT_AUTO) return "export: fract_bits must be 0..24 or GS_SPZ_FRACT_AUTO";
    if (s.compression_level < -1 || s.compression_level > 9) return "export: compression_level must be -1..9";
    if (s.slice_bytes != 0u && s.slice_bytes < kSpzSliceMin) return "export: slice_bytes must be 0 or at least 4096";
    return nullptr;
}
inline const char* spz_alive_refusal(uint64_t alive) {
    if (alive == 0u) return "export: no alive splat (an SPZ file holds at least one)";
    if (alive > gsm::kSpzMaxSplats) return "export: more than 10,000,000 alive splats (the SPZ readers' limit)";
    return nullptr;
}
// bytes of the gunzipped stream of n splats: the header and the six columns
inline uint64_t spz_body_bytes(uint64_t n, uint32_t shLevel) { return 16u + n * (19u + 3u * gsm::SpzShCoeffs(shLevel)); }

// what CSSelectionUpdate reads of a frame, and _SelectionRect
inline gsm::EditSelect edit_select_of(const gs_frame_params& p, const float rect[4]) {
    gsm::EditSelect S;
    memcpy(S.o2w, p.matrix_object_to_world, sizeof(S.o2w));
    memcpy(S.vp, p.matrix_vp, sizeof(S.vp));
    S.screenW = p.screen_w; S.screenH = p.screen_h;
    memcpy(S.rect, rect, sizeof(S.rect));
    return S;
}

// gs_renderer_edit_select_surface: (x0, y0) .. (x1, y1) inclusive, y down, clipped to a width x height target; w = h = 0 when nothing is left
// (the caller has refused x0 > x1 and y0 > y1)
inline gsm::PickSelect pick_select_of(int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t width, uint32_t height, uint32_t tag, int32_t subtract) {
    gsm::PickSelect S;
    memset(&S, 0, sizeof(S));
    S.stride = width; S.tag = tag; S.subtract = subtract ? 1u : 0u;
    const int64_t cx0 = x0 < 0 ? 0 : x0, cy0 = y0 < 0 ? 0 : y0;
    const int64_t cx1 = x1 >= (int64_t)width ? (int64_t)width - 1 : x1, cy1 = y1 >= (int64_t)height ? (int64_t)height - 1 : y1;
    if (cx0 > cx1 || cy0 > cy1) return S;
    S.x0 = (uint32_t)cx0; S.y0 = (uint32_t)cy0; S.w = (uint32_t)(cx1 - cx0 + 1); S.h = (uint32_t)(cy1 - cy0 + 1);
    return S;
}

// the three transforms: zeros, then _SelectionCenter and the two matrices (rotate, scale; center = null: translate, which reads neither) and the
// first deltaFloats of _SelectionDelta (3: translate, scale) / _SelectionDeltaRot (4: rotate)
inline gsm::EditXform edit_xform_of(const float* center, const float* o2w, const float* w2o, const float* delta, int deltaFloats) {
    gsm::EditXform X;
    memset(&X, 0, sizeof(X));
    if (center) {
        memcpy(X.center, center, sizeof(X.center));
        memcpy(X.o2w, o2w, sizeof(X.o2w));
        memcpy(X.w2o, w2o, sizeof(X.w2o));
    }
    memcpy(X.delta, delta, (size_t)deltaFloats * sizeof(float));
    return X;
}

inline void flatten_params(const gs_frame_params* p, gsm::FrameConsts& c) {
    memcpy(c.mv, p->matrix_mv, 12 * sizeof(float));
    memcpy(c.o2w, p->matrix_object_to_world, 12 * sizeof(float));
    memcpy(c.w2o, p->matrix_world_to_object, 12 * sizeof(float));
    memcpy(c.vp, p->matrix_vp, 16 * sizeof(float));
    gsm::FrameConstsFromProjection(c, p->proj_m00, p->proj_m11, p->screen_w); c.screenW = p->screen_w; c.screenH = p->screen_h;
    c.camx = p->cam_pos_world[0]; c.camy = p->cam_pos_world[1]; c.camz = p->cam_pos_world[2];
    c.splatScale = p->splat_scale; c.opacityScale = p->opacity_scale;
    c.shOrder = p->sh_order; c.shOnly = p->sh_only;
    c.nearClip = p->near_clip; c.farClip = p->far_clip;
    gsm::FrameConstsChunkCull(c);
}

} // namespace gs
