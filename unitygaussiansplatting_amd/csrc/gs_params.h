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

// what CSSelectionUpdate reads of a frame, and _SelectionRect
inline gsm::EditSelect edit_select_of(const gs_frame_params& p, const float rect[4]) {
    gsm::EditSelect S;
    memcpy(S.o2w, p.matrix_object_to_world, sizeof(S.o2w));
    memcpy(S.vp, p.matrix_vp, sizeof(S.vp));
    S.screenW = p.screen_w; S.screenH = p.screen_h;
    memcpy(S.rect, rect, sizeof(S.rect));
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
