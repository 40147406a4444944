// Test-only: the transform kernels' per-splat arithmetic (csrc/gs_device_math.h: EditTranslatePos, EditRotatePos, EditScalePos, EditRotateWord and the
// codec under it) compiled for the HOST, so that tests/test_transform_model.py can hold it to tests/transform_model.py bit for bit on a box without
// a GPU.  Never part of the shipped library.
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
// pos: n x 3 floats, words: n rotation words; delta3 for translate / scale, rot4 for rotate; out*: n x 3 floats, outW: n words
void th_eval(const float* pos, const uint32_t* words, uint32_t n, const float* center, const float* o2w16, const float* w2o16, const float* delta3,
             const float* rot4, float* outT, float* outR, float* outS, uint32_t* outW) {
    const gsm::EditXform X = gs::edit_xform_of(center, o2w16, w2o16, delta3, 3), XR = gs::edit_xform_of(center, o2w16, w2o16, rot4, 4);
    for (uint32_t i = 0; i < n; ++i) {
        const gsm::V3 p = { pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] };
        const gsm::V3 t = gsm::EditTranslatePos(X, p), r = gsm::EditRotatePos(XR, p), s = gsm::EditScalePos(X, p);
        outT[i * 3] = t.x; outT[i * 3 + 1] = t.y; outT[i * 3 + 2] = t.z;
        outR[i * 3] = r.x; outR[i * 3 + 1] = r.y; outR[i * 3 + 2] = r.z;
        outS[i * 3] = s.x; outS[i * 3 + 1] = s.y; outS[i * 3 + 2] = s.z;
        outW[i] = gsm::EditRotateWord(XR, words[i]);
    }
}

// q: n x 4 floats; packed = PackSmallest3Rotation(q), enc = EncodeQuatToNorm10(packed), dec = DecodeRotation(enc)
void th_codec(const float* q, uint32_t n, float* packed, uint32_t* enc, float* dec) {
    for (uint32_t i = 0; i < n; ++i) {
        const gsm::V4 p = gsm::PackSmallest3Rotation({ q[i * 4], q[i * 4 + 1], q[i * 4 + 2], q[i * 4 + 3] });
        packed[i * 4] = p.x; packed[i * 4 + 1] = p.y; packed[i * 4 + 2] = p.z; packed[i * 4 + 3] = p.w;
        enc[i] = gsm::EncodeQuatToNorm10(p);
        const gsm::V4 d = gsm::DecodeRotation(enc[i]);
        dec[i * 4] = d.x; dec[i * 4 + 1] = d.y; dec[i * 4 + 2] = d.z; dec[i * 4 + 3] = d.w;
    }
}
}
