// Test-only: the rigid rotate / scale of the selection compiled for the HOST -- the per-call part (gs::edit_rigid_rotate_of, csrc/gs_params.h) and the
// per-splat arithmetic the RIGID kernels call (gsm::EditRigidRotateWord, EditRigidRotateSH, EditRigidScale, csrc/gs_device_math.h) -- so that
// tests/test_rigid_model.py can hold them to tests/rigid_model.py bit for bit on a box without a GPU, and to the shipped merge (BakeSplatTransform).
// Never part of the shipped library.
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
// out: L 9 floats (row-major 3x3), q 4, bands 83 (sh1, sh2, sh3); returns 0, or 1 when the arguments are refused
int rh_xform(const float* o2w16, const float* w2o16, const float* delta4, float* L9, float* q4, float* bands83) {
    gsm::EditRigid G;
    float L[12];
    if (gs::edit_rigid_rotate_of(o2w16, w2o16, delta4, G, L)) return 1;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) L9[i * 3 + j] = L[i * 4 + j];
    memcpy(q4, G.q, sizeof(G.q));
    memcpy(bands83, &G.sh, sizeof(G.sh));
    return 0;
}

// the rigid rotate of n splats: words n, sh n x 48 floats (192-byte records); outSH must hold the records beforehand (their last 12 bytes are not written)
int rh_rotate(const float* o2w16, const float* w2o16, const float* delta4, const uint32_t* words, const float* sh, uint32_t n, uint32_t* outW, float* outSH) {
    gsm::EditRigid G;
    float L[12];
    if (gs::edit_rigid_rotate_of(o2w16, w2o16, delta4, G, L)) return 1;
    for (uint32_t i = 0; i < n; ++i) {
        outW[i] = gsm::EditRigidRotateWord(G, words[i]);
        gsm::EditRigidRotateSH(G, sh + (size_t)i * 48, outSH + (size_t)i * 48);
    }
    return 0;
}

// the same splats through the shipped merge: BakeSplatTransform(m = L, rot = q_L, scale = 1) of a splat whose rot is the decoded word; outQ: the
// quaternion it leaves (n x 4), outW: the encoder's word of it, outSH: n x 45 coefficients
int rh_bake(const float* o2w16, const float* w2o16, const float* delta4, const uint32_t* words, const float* sh, uint32_t n, float* outQ, uint32_t* outW, float* outSH) {
    gsm::EditRigid G;
    float L[12];
    if (gs::edit_rigid_rotate_of(o2w16, w2o16, delta4, G, L)) return 1;
    const float one[3] = { 1.0f, 1.0f, 1.0f };
    for (uint32_t i = 0; i < n; ++i) {
        gsm::SplatFull s;
        memset(&s, 0, sizeof(s));
        s.rot = gsm::DecodeRotation(words[i]);
        s.scale = { 1.0f, 1.0f, 1.0f };
        for (int k = 0; k < 15; ++k) s.sh[k] = { sh[(size_t)i * 48 + 3 * k], sh[(size_t)i * 48 + 3 * k + 1], sh[(size_t)i * 48 + 3 * k + 2] };
        gsm::BakeSplatTransform(s, L, G.q, one, G.sh);
        outQ[i * 4] = s.rot.x; outQ[i * 4 + 1] = s.rot.y; outQ[i * 4 + 2] = s.rot.z; outQ[i * 4 + 3] = s.rot.w;
        outW[i] = gsm::EncodeQuatToNorm10(gsm::PackSmallest3Rotation(s.rot));
        for (int k = 0; k < 15; ++k) { outSH[(size_t)i * 45 + 3 * k] = s.sh[k].x; outSH[(size_t)i * 45 + 3 * k + 1] = s.sh[k].y; outSH[(size_t)i * 45 + 3 * k + 2] = s.sh[k].z; }
    }
    return 0;
}

// the uniform scale: scales n x 3 -> out n x 3; returns whether delta3 counts as uniform
int rh_scale(const float* delta3, const float* scales, uint32_t n, float* out) {
    if (!gs::edit_rigid_scale_uniform(delta3)) return 0;
    const gsm::EditRigid G = gs::edit_rigid_scale_of(delta3);
    for (uint32_t i = 0; i < n; ++i) {
        const gsm::V3 v = gsm::EditRigidScale(G, { scales[i * 3], scales[i * 3 + 1], scales[i * 3 + 2] });
        out[i * 3] = v.x; out[i * 3 + 1] = v.y; out[i * 3 + 2] = v.z;
    }
    return 1;
}
}
