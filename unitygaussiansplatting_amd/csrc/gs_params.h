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

// The rigid rotate / scale of the selection (gs_renderer_edit_set_rigid_transforms): what the kernel needs besides the
// EditXform, made once per call.  Each function returns what is wrong with its arguments, or null.
//
// edit_rigid_rotate_of -- the linear part of CSRotateSelection's position map is L = W2O3 . R(d) . O2W3 (3x3 parts, d = the delta quaternion).
// Operation order (what makes the bits a function of this text; tests/rigid_model.py follows it):
//   1. d = (x, y, z, w) widened to fp64; n = sqrt(((x x + y y) + z z) + w w); refused unless 0 < n < inf; d = d / n, four divisions
//   2. R(d) in fp64: R00 = 1 - 2 (yy + zz), R01 = 2 (xy - zw), R02 = 2 (xz + yw), R10 = 2 (xy + zw), R11 = 1 - 2 (xx + zz), R12 = 2 (yz - xw),
//      R20 = 2 (xz - yw), R21 = 2 (yz + xw), R22 = 1 - 2 (xx + yy); every product, sum and difference rounds once, as written
//   3. T = R . O2W3, then L = W2O3 . T, in fp64: entry (i, j) = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]
//      (an O2W3 row whose squared length (x x + y y) + z z, in fp64, is not in (0, inf) is refused first)
//   4. L rounded to fp32, entry by entry (Lf; handed out as rows of 4 with a zero fourth column)
//   5. G.sh = CalcSHRot(Lf): the band matrices of Lf's ROW-NORMALISED form M (gsm::SHRotMatrix, fp32) -- the reference's answer for a matrix
//      that is not a pure rotation (a scaled or sheared tool frame)
//   6. G.q = the quaternion of M, in fp64 from M's fp32 entries, by the largest-diagonal method with strict comparisons:
//        t = (M00 + M11) + M22
//        t > 0:                    s = sqrt(t + 1) 2;                 w = s / 4;            x = (M21 - M12) / s;  y = (M02 - M20) / s;  z = (M10 - M01) / s
//        else M00 > M11, M00 > M22: s = sqrt(((1 + M00) - M11) - M22) 2;  w = (M21 - M12) / s;  x = s / 4;            y = (M01 + M10) / s;  z = (M02 + M20) / s
//        else M11 > M22:           s = sqrt(((1 + M11) - M00) - M22) 2;  w = (M02 - M20) / s;  x = (M01 + M10) / s;  y = s / 4;            z = (M12 + M21) / s
//        else:                     s = sqrt(((1 + M22) - M00) - M11) 2;  w = (M10 - M01) / s;  x = (M02 + M20) / s;  y = (M12 + M21) / s;  z = s / 4
//      then divided by sqrt(((x x + y y) + z z) + w w) and rounded to fp32 once.  (For a mirrored M the result is this text's, not a rotation.)
inline const char* edit_rigid_rotate_of(const float* o2w, const float* w2o, const float* delta, gsm::EditRigid& G, float* L12) {
    memset(&G, 0, sizeof(G));
    G.s = 1.0f;
    double d[4] = { (double)delta[0], (double)delta[1], (double)delta[2], (double)delta[3] };
    const double n = sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]);
    if (!(n > 0.0) || !(n <= 1.7976931348623157e308)) return "rotate: the delta quaternion has a zero or non-finite norm";
    for (int k = 0; k < 4; ++k) d[k] = d[k] / n;
    double A[3][3], B[3][3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { A[r][c] = (double)o2w[r * 4 + c]; B[r][c] = (double)w2o[r * 4 + c]; }
        const double len2 = (A[r][0] * A[r][0] + A[r][1] * A[r][1]) + A[r][2] * A[r][2];
        if (!(len2 > 0.0) || !(len2 <= 1.7976931348623157e308)) return "rotate: local_to_world has a zero or non-finite row";
    }
    const double x = d[0], y = d[1], z = d[2], w = d[3];
    const double R[3][3] = { { 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w) },
                             { 2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w) },
                             { 2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y) } };
    double T[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[i][j] = (R[i][0] * A[0][j] + R[i][1] * A[1][j]) + R[i][2] * A[2][j];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) L12[i * 4 + j] = (float)((B[i][0] * T[0][j] + B[i][1] * T[1][j]) + B[i][2] * T[2][j]);
        L12[i * 4 + 3] = 0.0f;
    }
    gsm::CalcSHRot(L12, G.sh);
    float Mf[3][3];
    gsm::SHRotMatrix(L12, Mf);
    double M[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = (double)Mf[i][j];
    const double t = (M[0][0] + M[1][1]) + M[2][2];
    double q[4];                                                   // x y z w
    if (t > 0.0) {
        const double s = sqrt(t + 1.0) * 2.0;
        q[3] = s / 4.0; q[0] = (M[2][1] - M[1][2]) / s; q[1] = (M[0][2] - M[2][0]) / s; q[2] = (M[1][0] - M[0][1]) / s;
    } else if (M[0][0] > M[1][1] && M[0][0] > M[2][2]) {
        const double s = sqrt(((1.0 + M[0][0]) - M[1][1]) - M[2][2]) * 2.0;
        q[3] = (M[2][1] - M[1][2]) / s; q[0] = s / 4.0; q[1] = (M[0][1] + M[1][0]) / s; q[2] = (M[0][2] + M[2][0]) / s;
    } else if (M[1][1] > M[2][2]) {
        const double s = sqrt(((1.0 + M[1][1]) - M[0][0]) - M[2][2]) * 2.0;
        q[3] = (M[0][2] - M[2][0]) / s; q[0] = (M[0][1] + M[1][0]) / s; q[1] = s / 4.0; q[2] = (M[1][2] + M[2][1]) / s;
    } else {
        const double s = sqrt(((1.0 + M[2][2]) - M[0][0]) - M[1][1]) * 2.0;
        q[3] = (M[1][0] - M[0][1]) / s; q[0] = (M[0][2] + M[2][0]) / s; q[1] = (M[1][2] + M[2][1]) / s; q[2] = s / 4.0;
    }
    const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) G.q[k] = (float)(q[k] / qn);
    return nullptr;
}
// the uniform handle of the scale tool: the three components of the delta are equal as floats (s s s); the linear part is then s I whatever
// O2W is, and a selected splat's three scales become |s| times what they were at mouse down.  A non-uniform delta leaves splat sizes alone.
inline bool edit_rigid_scale_uniform(const float* delta) { return delta[0] == delta[1] && delta[1] == delta[2]; }
inline gsm::EditRigid edit_rigid_scale_of(const float* delta) {
    gsm::EditRigid G;
    memset(&G, 0, sizeof(G));
    G.s = delta[0];
    return G;
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
