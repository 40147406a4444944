// gs_device_math.h -- per-splat arithmetic of the gfx950 kernels (decode, sort key, view data).
//
// Everything here is plain IEEE fp32 with explicit fmaf() and is compiled with -ffp-contract=off, so the
// numbers are a function of the source only ("canonical arithmetic").  The functions are
// __host__ __device__ so that tests/test_host_math.py can compile this header with g++ and compare it with
// the oracle bit for bit on the CPU box; the shipped library only ever calls them from device code.
//
// Reference lines restated (paths relative to /root/reference/package/Shaders/):
//   GaussianSplatting.hlsl :5-11 InvSquareCentered01, :29-53 CalcMatrixFromRotationScale/CalcCovariance3D,
//   :56-90 CalcCovariance2D, :113-127,183-194 Morton texel address, :130-179 ShadeSH, :219-229 DecodeRotation,
//   :261-300 DecodePacked_*, :325-421 LoadUShort/LoadUInt/LoadAndDecodeVector/LoadSplatPos, :428-608 LoadSplatData
//   SplatUtilities.compute :52-57 FloatToSortableUint, :107-162 DecomposeCovariance, :189-252 CSCalcViewData,
//   :279-296 CSUpdateEditData's bounds, :400-416 CSSelectionUpdate's hit test, :425-521 CSTranslateSelection / CSRotateSelection /
//   CSScaleSelection with GaussianSplatting.hlsl :13-22 QuatRotateVector / QuatMul, :230-259 PackSmallest3Rotation, :301-304
//   EncodeQuatToNorm10 (the edit kernels: gs_edit.hip)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#define GS_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#include <cstring>
#define GS_HD inline
#endif

#ifndef GS_CULL_EXTENT
#define GS_CULL_EXTENT 2.8285f     // 2 sqrt(2), rounded up: see the early cull in CalcViewGeom
#endif

namespace gsm {

struct AssetView {              // device (or, in the host test, host) pointers to the five blobs
    const uint8_t* pos;
    const uint8_t* other;
    const uint8_t* color;
    const uint8_t* sh;
    const uint8_t* chunk;
    uint32_t n, posFmt, scaleFmt, colorFmt, shFmt, chunkCount;
};

struct FrameConsts {            // gs_frame_params flattened for kernel argument passing
    float mv[12];               // rows 0..2 of _MatrixMV
    float o2w[12];              // rows 0..2 of _MatrixObjectToWorld
    float w2o[12];              // rows 0..2 of _MatrixWorldToObject (3x3 part used)
    float vp[16];               // UNITY_MATRIX_VP
    float limX, limY, focal;    // 1.3 tanFovX, 1.3 tanFovY, W P00 / 2 of CalcCovariance2D: per-frame constants, see FrameConstsFromProjection
    float cullKx, cullKy, cullMx, cullMy;   // whole-chunk frustum cull (ChunkOutside), see FrameConstsChunkCull
    uint32_t cullOn;
    float screenW, screenH;
    float camx, camy, camz;
    float splatScale, opacityScale;
    uint32_t shOrder, shOnly;
    float nearClip, farClip;
};

// Edit state CSCalcViewData consults (SplatUtilities.compute:91-105): _SplatDeletedBits / _SplatBitsValid and _SplatCutouts
struct EditView {
    const uint32_t* deletedBits;    // ceil(n/32) words, or null (_SplatBitsValid = 0)
    const uint32_t* cutouts;        // cutoutCount x 17 dwords: float4x4 (rows of 4) + typeAndFlags
    uint32_t cutoutCount;
    // _SplatSelectedBits of the draw (RenderGaussianSplats.shader:63-73), ceil(n/32) words: the selection a splat frame highlights.  Null whenever the
    // highlight is off or there are no edit buffers; only the highlight builds of calc_view read it (SplatSelected below).
    const uint32_t* selectedBits = nullptr;
};

// The camera-only part of CalcCovariance2D (GaussianSplatting.hlsl:62-72), evaluated once per frame on the host with the
// same fp32 operations the shader performs per splat (aspect = P00/P11; tanFovX = 1/P00; tanFovY = 1/(P11 aspect) -- which is
// 1/P00 again, a quirk of the reference that is kept; focal = W P00 / 2): three IEEE divisions less per splat.
GS_HD void FrameConstsFromProjection(FrameConsts& c, float p00, float p11, float screenW) {
    const float aspect = p00 / p11;
    const float tanFovX = 1.0f / p00;
    const float tanFovY = 1.0f / (p11 * aspect);
    c.limX = 1.3f * tanFovX;
    c.limY = 1.3f * tanFovY;
    c.focal = screenW * p00 / 2.0f;
}

struct ViewData { float pos[4]; float axis1[2]; float axis2[2]; uint32_t color[2]; };   // 40 B SplatViewData

// ---- bit casts / half ---------------------------------------------------------------------------
GS_HD uint32_t f2u(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}
GS_HD float u2f(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
GS_HD float f16tof32(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half((unsigned short)(h & 0xffffu)));
#else
    h &= 0xffffu;
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) x = sign;
        else { int s = 0; while (!(m & 0x400u)) { m <<= 1; s++; } m &= 0x3ffu; x = sign | ((uint32_t)(113 - s) << 23) | (m << 13); }
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e + 112u) << 23) | (m << 13);
    return u2f(x);
#endif
}
GS_HD uint32_t f32tof16(float f) {     // round to nearest even
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__half_as_ushort(__float2half_rn(f));
#else
    uint32_t x = f2u(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return sign | 0x7e00u;
    if (x >= 0x477ff000u) return sign | 0x7c00u;
    if (x < 0x38800000u) {
        if (x < 0x33000000u) return sign;
        const uint32_t e = x >> 23, m = (x & 0x7fffffu) | 0x800000u, shift = 126u - e;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (r & 1u))) r++;
        return sign | r;
    }
    uint32_t r = x - 0x38000000u;
    const uint32_t rem = r & 0x1fffu;
    r >>= 13;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return sign | r;
#endif
}

// ---- scalar helpers -----------------------------------------------------------------------------
GS_HD float lerpf(float a, float b, float t) { return fmaf(t, b - a, a); }
GS_HD float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
GS_HD bool finite32(float x) { return fabsf(x) <= 3.4028234663852886e38f; }
GS_HD float sgn(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }
GS_HD float dot3f(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }
GS_HD float dot2f(float ax, float ay, float bx, float by) { return fmaf(ay, by, ax * bx); }
// row r of mul(M, float4(v,1)) for a matrix stored as rows of 4
GS_HD float mrow(const float* m, int r, float x, float y, float z) {
    return fmaf(m[r * 4 + 2], z, fmaf(m[r * 4 + 1], y, fmaf(m[r * 4 + 0], x, m[r * 4 + 3])));
}
GS_HD float mrow3(const float* m, int r, float x, float y, float z) {
    return fmaf(m[r * 4 + 2], z, fmaf(m[r * 4 + 1], y, m[r * 4 + 0] * x));
}

GS_HD uint32_t FloatToSortableUint(float f) {
    const uint32_t fu = f2u(f);
    const uint32_t mask = (uint32_t)(-(int32_t)(fu >> 31)) | 0x80000000u;
    return fu ^ mask;
}

// ---- raw loads (2-byte aligned addresses, stitched from aligned dwords like the HLSL) -------------
GS_HD uint32_t ld32a(const uint8_t* p, uint64_t a) { return *(const uint32_t*)(p + a); }            // a % 4 == 0
GS_HD uint32_t LoadUInt(const uint8_t* p, uint64_t a) {
    const uint64_t aa = a & ~(uint64_t)3;
    uint32_t v = ld32a(p, aa);
    if (a != aa) { const uint32_t v1 = ld32a(p, aa + 4); v = (v >> 16) | (v1 << 16); }
    return v;
}
GS_HD uint32_t LoadUShort(const uint8_t* p, uint64_t a) {
    const uint64_t aa = a & ~(uint64_t)3;
    uint32_t v = ld32a(p, aa);
    if (a != aa) v >>= 16;
    return v & 0xffffu;
}

#define GS_R63 (1.0f / 63.0f)
#define GS_R31 (1.0f / 31.0f)
#define GS_R2047 (1.0f / 2047.0f)
#define GS_R1023 (1.0f / 1023.0f)
#define GS_R65535 (1.0f / 65535.0f)
#define GS_R255 (1.0f / 255.0f)

struct V3 { float x, y, z; };
struct V4 { float x, y, z, w; };
// (r, g) of a colour as a 2-vector: on the device its fp32 multiplies / fmas are ONE packed instruction (v_pk_mul_f32 /
// v_pk_fma_f32 run two IEEE operations per issue slot on gfx950) -- same results as the scalar forms, element by element.
#if defined(__clang__)
typedef float F2 __attribute__((ext_vector_type(2)));
#else       // a host compiler without vector extensions (the header is also compiled by g++ in tests): the same arithmetic, element by element
struct F2 { float x, y; };
inline F2 operator*(F2 a, F2 b) { return F2{ a.x * b.x, a.y * b.y }; }
inline F2 operator-(F2 a, F2 b) { return F2{ a.x - b.x, a.y - b.y }; }
inline F2 operator-(F2 a) { return F2{ -a.x, -a.y }; }
inline F2& operator+=(F2& a, F2 b) { a.x += b.x; a.y += b.y; return a; }
#endif
struct RGB { F2 rg; float b; };
GS_HD F2 fma2(F2 a, F2 b, F2 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_elementwise_fma(a, b, c);
#else
    return F2{ fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y) };
#endif
}

GS_HD V3 Dec_6_5_5(uint32_t e) { return { (float)(e & 63) * GS_R63, (float)((e >> 6) & 31) * GS_R31, (float)((e >> 11) & 31) * GS_R31 }; }
GS_HD V3 Dec_5_6_5(uint32_t e) { return { (float)(e & 31) * GS_R31, (float)((e >> 5) & 63) * GS_R63, (float)((e >> 11) & 31) * GS_R31 }; }
GS_HD V3 Dec_11_10_11(uint32_t e) { return { (float)(e & 2047) * GS_R2047, (float)((e >> 11) & 1023) * GS_R1023, (float)((e >> 21) & 2047) * GS_R2047 }; }
GS_HD V3 Dec_16_16_16(uint32_t e0, uint32_t e1) { return { (float)(e0 & 65535) * GS_R65535, (float)(e0 >> 16) * GS_R65535, (float)(e1 & 65535) * GS_R65535 }; }

GS_HD uint32_t vecStride(uint32_t fmt) { return fmt == 0 ? 12u : (fmt == 1 ? 6u : (fmt == 2 ? 4u : 2u)); }

GS_HD V3 LoadVec(const uint8_t* buf, uint64_t a, uint32_t fmt) {
    if (fmt == 0) return { u2f(LoadUInt(buf, a)), u2f(LoadUInt(buf, a + 4)), u2f(LoadUInt(buf, a + 8)) };
    if (fmt == 1) return Dec_16_16_16(LoadUInt(buf, a), LoadUShort(buf, a + 4));
    if (fmt == 2) return Dec_11_10_11(LoadUInt(buf, a));
    return Dec_6_5_5(LoadUShort(buf, a));
}

// The same values as LoadVec for a compile-time format, with every load unconditional (a load inside a branch is waited for
// at the end of the branch, which serialises a streaming kernel's loads): unaligned 6- and 2-byte records take the two aligned
// dwords around them and select (the blobs carry >= 4 readable bytes after the last record).
template <int FMT> struct RawVec { uint32_t d[FMT == 0 ? 3 : (FMT == 1 ? 2 : 1)]; };
template <int FMT> GS_HD RawVec<FMT> LoadRawT(const uint8_t* buf, uint64_t a) {            // the loads alone (so that a caller can issue many before it decodes)
    RawVec<FMT> r;
    if (FMT == 0) { r.d[0] = ld32a(buf, a); r.d[FMT == 0 ? 1 : 0] = ld32a(buf, a + 4); r.d[FMT == 0 ? 2 : 0] = ld32a(buf, a + 8); return r; }
    const uint64_t aa = a & ~(uint64_t)3;
    r.d[0] = ld32a(buf, aa);
    if (FMT == 1) r.d[FMT == 1 ? 1 : 0] = ld32a(buf, aa + 4);
    return r;
}
template <int FMT> GS_HD V3 DecodeRawT(const RawVec<FMT>& r, uint64_t a) {
    if (FMT == 0) return { u2f(r.d[0]), u2f(r.d[FMT == 0 ? 1 : 0]), u2f(r.d[FMT == 0 ? 2 : 0]) };
    if (FMT == 2) return Dec_11_10_11(r.d[0]);
    const bool odd = (a & 2u) != 0;
    if (FMT == 3) return Dec_6_5_5(odd ? (r.d[0] >> 16) : (r.d[0] & 0xffffu));
    const uint32_t d0 = r.d[0], d1 = r.d[FMT == 1 ? 1 : 0];
    return Dec_16_16_16(odd ? ((d0 >> 16) | (d1 << 16)) : d0, odd ? (d1 >> 16) : (d1 & 0xffffu));
}
template <int FMT> GS_HD V3 LoadVecT(const uint8_t* buf, uint64_t a) { return DecodeRawT<FMT>(LoadRawT<FMT>(buf, a), a); }
template <int FMT> GS_HD uint32_t vecStrideT() { return FMT == 0 ? 12u : (FMT == 1 ? 6u : (FMT == 2 ? 4u : 2u)); }

// What a kernel knows of an asset's layout when it is compiled.  A field of kFmtRuntime is read from the AssetView as it always
// was; any other value stands in for the AssetView's field, so the loaders below fold to the one format's loads and strides --
// the same expressions in the same order, with the branches of the other formats gone.  CHUNKED: 1 = every splat's chunk exists
// (chunkCount covers all of n), 0 = the asset has no chunk blob, kFmtRuntime = compare the chunk index with chunkCount.
// Whoever launches a kernel built on fixed formats checks that the AssetView really has them (gs_view.hip).
constexpr int kFmtRuntime = -1;
template <int POS, int SCALE, int COLOR, int SH, int CHUNKED> struct AssetFormats {
    static constexpr int kPos = POS, kScale = SCALE, kColor = COLOR, kSH = SH, kChunked = CHUNKED;
    static GS_HD uint32_t posFmt(const AssetView& a) { return POS == kFmtRuntime ? a.posFmt : (uint32_t)POS; }
    static GS_HD uint32_t scaleFmt(const AssetView& a) { return SCALE == kFmtRuntime ? a.scaleFmt : (uint32_t)SCALE; }
    static GS_HD uint32_t colorFmt(const AssetView& a) { return COLOR == kFmtRuntime ? a.colorFmt : (uint32_t)COLOR; }
    static GS_HD uint32_t shFmt(const AssetView& a) { return SH == kFmtRuntime ? a.shFmt : (uint32_t)SH; }
    static GS_HD bool chunked(const AssetView& a, uint32_t ci) { return CHUNKED == kFmtRuntime ? ci < a.chunkCount : CHUNKED != 0; }
};
typedef AssetFormats<kFmtRuntime, kFmtRuntime, kFmtRuntime, kFmtRuntime, kFmtRuntime> RuntimeFormats;

// chunk de-normalisation of a decoded position (LoadSplatPos, GaussianSplatting.hlsl:394-421)
GS_HD V3 ChunkLerpPos(const AssetView& a, V3 p, uint32_t ci) {
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        p.x = lerpf(u2f(ld32a(c, 16)), u2f(ld32a(c, 20)), p.x);
        p.y = lerpf(u2f(ld32a(c, 24)), u2f(ld32a(c, 28)), p.y);
        p.z = lerpf(u2f(ld32a(c, 32)), u2f(ld32a(c, 36)), p.z);
    }
    return p;
}
template <int FMT> GS_HD V3 LoadSplatPosChunkT(const AssetView& a, uint32_t idx, uint32_t ci) {
    return ChunkLerpPos(a, LoadVecT<FMT>(a.pos, (uint64_t)idx * vecStrideT<FMT>()), ci);
}

struct ChunkRaw { uint32_t w[16]; };    // colR,colG,colB,colA, posX(2),posY(2),posZ(2), sclX..Z, shR..B
GS_HD ChunkRaw LoadChunk(const uint8_t* chunk, uint32_t ci) {
    ChunkRaw c;
    const uint32_t* p = (const uint32_t*)(chunk + (uint64_t)ci * 64);
#pragma unroll
    for (int k = 0; k < 16; ++k) c.w[k] = p[k];     // uniform per 256-splat block: becomes one scalar s_load_dwordx16
    return c;
}

// LoadSplatPos (GaussianSplatting.hlsl:394-421); ci = idx >> 8, passed separately so that a caller whose workgroup is aligned
// to the 256-splat chunks can hand in a wave-uniform value (the ChunkInfo loads then become scalar loads)
GS_HD V3 LoadSplatPosChunk(const AssetView& a, uint32_t idx, uint32_t ci) {
    V3 p = LoadVec(a.pos, (uint64_t)idx * vecStride(a.posFmt), a.posFmt);
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        p.x = lerpf(u2f(ld32a(c, 16)), u2f(ld32a(c, 20)), p.x);
        p.y = lerpf(u2f(ld32a(c, 24)), u2f(ld32a(c, 28)), p.y);
        p.z = lerpf(u2f(ld32a(c, 32)), u2f(ld32a(c, 36)), p.z);
    }
    return p;
}
GS_HD V3 LoadSplatPos(const AssetView& a, uint32_t idx) { return LoadSplatPosChunk(a, idx, idx >> 8); }

// CSCalcDistances body (SplatUtilities.compute:76-81): key of the splat `origIdx` under sort-matrix row 2
GS_HD uint32_t SortKeyOf(const V3& p, float m20, float m21, float m22, float m23) {
    const float z = fmaf(m22, p.z, fmaf(m21, p.y, fmaf(m20, p.x, m23)));
    return FloatToSortableUint(z);
}
GS_HD uint32_t SortKey(const AssetView& a, uint32_t origIdx, float m20, float m21, float m22, float m23) {
    return SortKeyOf(LoadSplatPos(a, origIdx), m20, m21, m22, m23);
}

GS_HD void SplatIndexToPixelIndex(uint32_t idx, uint32_t& x, uint32_t& y) {
    uint32_t t = idx;
    t = (t & 0xFF) | ((t & 0xFE) << 7);
    t &= 0x5555;
    t = (t ^ (t >> 1)) & 0x3333;
    t = (t ^ (t >> 2)) & 0x0f0f;
    const uint32_t tile = idx >> 8;
    x = (tile & 127u) * 16 + (t & 0xF);
    y = (tile >> 7) * 16 + (t >> 8);
}

GS_HD float InvSquareCentered01(float x) {
    x -= 0.5f;
    x *= 0.5f;
    x = sqrtf(fabsf(x)) * sgn(x);
    return x + 0.5f;
}

GS_HD V4 DecodeRotation(uint32_t enc) {
    const float px = (float)(enc & 1023) * GS_R1023, py = (float)((enc >> 10) & 1023) * GS_R1023, pz = (float)((enc >> 20) & 1023) * GS_R1023;
    const uint32_t idx = enc >> 30;
    const float SQRT2 = 1.41421356237f, INV_SQRT2 = 0.70710678118f;
    const float qx = fmaf(px, SQRT2, -INV_SQRT2), qy = fmaf(py, SQRT2, -INV_SQRT2), qz = fmaf(pz, SQRT2, -INV_SQRT2);
    const float qw = sqrtf(1.0f - sat(dot3f(qx, qy, qz, qx, qy, qz)));
    V4 q = { qx, qy, qz, qw };
    if (idx == 0) q = { qw, qx, qy, qz };
    if (idx == 1) q = { qx, qw, qy, qz };
    if (idx == 2) q = { qx, qy, qw, qz };
    return q;
}

// QuatMul(a, b) (GaussianSplatting.hlsl:19-22): every product and sum on its own, in the order of the reference's text
GS_HD V4 QuatMul(const V4& qa, const V4& qb) {
    V4 r;
    r.x = (qa.w * qb.x + (qa.x * qb.w + qa.y * qb.z)) - qa.z * qb.y;
    r.y = (qa.w * qb.y + (qa.y * qb.w + qa.z * qb.x)) - qa.x * qb.z;
    r.z = (qa.w * qb.z + (qa.z * qb.w + qa.x * qb.y)) - qa.y * qb.x;
    r.w = (qa.w * qb.w + -(qa.x * qb.x + qa.y * qb.y)) - qa.z * qb.z;
    return r;
}

// QuatRotateVector(v, r) (GaussianSplatting.hlsl:13-17): t = 2 cross(r.xyz, v); v + r.w t + cross(r.xyz, t)
GS_HD V3 QuatRotateVector(const V3& v, const V4& r) {
    const float tx = 2.0f * (r.y * v.z - r.z * v.y), ty = 2.0f * (r.z * v.x - r.x * v.z), tz = 2.0f * (r.x * v.y - r.y * v.x);
    const float cx = r.y * tz - r.z * ty, cy = r.z * tx - r.x * tz, cz = r.x * ty - r.y * tx;
    return { (v.x + r.w * tx) + cx, (v.y + r.w * ty) + cy, (v.z + r.w * tz) + cz };
}

// PackSmallest3Rotation (GaussianSplatting.hlsl:230-259): the strict > chain (the first of equal magnitudes wins; a NaN never does), the
// swizzles, q.w >= 0 ? 1 : -1 (so -0 counts as positive and a NaN as negative), (three * sqrt(2.0)) * 0.5 + 0.5 as three fp32 operations
// with sqrt(2.0) the fp32 square root (the halving is exact, so a fused last step gives the same bits), index / 3.0 as a division.
GS_HD V4 PackSmallest3Rotation(V4 q) {
    const float ax = fabsf(q.x), ay = fabsf(q.y), az = fabsf(q.z), aw = fabsf(q.w);
    int index = 0;
    float maxV = ax;
    if (ay > maxV) { index = 1; maxV = ay; }
    if (az > maxV) { index = 2; maxV = az; }
    if (aw > maxV) { index = 3; maxV = aw; }
    if (index == 0) q = { q.y, q.z, q.w, q.x };
    if (index == 1) q = { q.x, q.z, q.w, q.y };
    if (index == 2) q = { q.x, q.y, q.w, q.z };
    const float s = (q.w >= 0.0f) ? 1.0f : -1.0f, SQRT2 = 1.41421356237f;
    V4 r;
    r.x = ((q.x * s) * SQRT2) * 0.5f + 0.5f;
    r.y = ((q.y * s) * SQRT2) * 0.5f + 0.5f;
    r.z = ((q.z * s) * SQRT2) * 0.5f + 0.5f;
    r.w = (float)index / 3.0f;
    return r;
}

// EncodeQuatToNorm10 (GaussianSplatting.hlsl:301-304): truncating conversions of v * 1023.5 / v.w * 3.5.  One deviation: every field is
// clamped to its range first (a NaN becomes 0) -- a delta quaternion that is not of unit length takes `three` out of [0, 1], where the
// reference's conversion is undefined or spills into the next field; for every value inside the range the result is the reference's.
GS_HD uint32_t EncodeNormField(float v, float scale, float hi) { return (uint32_t)fminf(fmaxf(v * scale, 0.0f), hi); }
GS_HD uint32_t EncodeQuatToNorm10(const V4& v) {
    return EncodeNormField(v.x, 1023.5f, 1023.0f) | (EncodeNormField(v.y, 1023.5f, 1023.0f) << 10) | (EncodeNormField(v.z, 1023.5f, 1023.0f) << 20) |
           (EncodeNormField(v.w, 3.5f, 3.0f) << 30);
}

// SH coefficient k (1..15) of the splat whose SH record starts at `sp`, before chunk de-normalisation
GS_HD V3 LoadSH(const uint8_t* sp, uint32_t shFormat, int k) {
    if (shFormat == 0) return { u2f(ld32a(sp, (k - 1) * 12)), u2f(ld32a(sp, (k - 1) * 12 + 4)), u2f(ld32a(sp, (k - 1) * 12 + 8)) };
    if (shFormat == 2) return Dec_11_10_11(ld32a(sp, (k - 1) * 4));
    if (shFormat == 3) return Dec_5_6_5(LoadUShort(sp, (uint64_t)(k - 1) * 2));
    // fp16 (Float16 and Cluster* tables)
    return { f16tof32(LoadUShort(sp, (uint64_t)(k - 1) * 6)), f16tof32(LoadUShort(sp, (uint64_t)(k - 1) * 6 + 2)), f16tof32(LoadUShort(sp, (uint64_t)(k - 1) * 6 + 4)) };
}

// the same coefficient as (rg, b); the 5.6.5 decode's multiplies are packed
GS_HD RGB LoadSHrgb(const uint8_t* sp, uint32_t shFormat, int k) {
    if (shFormat == 3) {
        const uint32_t e = LoadUShort(sp, (uint64_t)(k - 1) * 2);
        return { F2{ (float)(e & 31), (float)((e >> 5) & 63) } * F2{ GS_R31, GS_R63 }, (float)((e >> 11) & 31) * GS_R31 };
    }
    const V3 v = LoadSH(sp, shFormat, k);
    return { F2{ v.x, v.y }, v.z };
}

GS_HD uint32_t shStrideOf(uint32_t shFormat) { return shFormat == 0 ? 192u : (shFormat == 2 ? 60u : (shFormat == 3 ? 32u : 96u)); }

#define GS_SH_C1 0.4886025f

// Where the raw (still chunk-normalised) SH coefficients of a splat come from: straight from the asset blob here; the
// view kernel substitutes a reader of its LDS-staged copy (gs_view.hip).  begin() receives the record's address.
struct SHFromBlob {
    const uint8_t* sp; uint32_t fmt;
    GS_HD void begin(const uint8_t* p, uint32_t f) { sp = p; fmt = f; }
    GS_HD V3 load(int k) const { return LoadSH(sp, fmt, k); }
    GS_HD RGB load_rgb(int k) const { return LoadSHrgb(sp, fmt, k); }
};

// Whole-chunk cull (per-frame path only).  A chunk's 256 splats lie in the box [posMin, posMax] of its ChunkInfo and are no
// larger than its scale maximum, so if all 8 corners of the box are on the outer side of one frustum plane -- pushed out
// by a bound on the footprint radius -- no splat of the chunk can be drawn and its workgroup stops before decoding anything.
// Footprint half extent <= 2 sqrt(2) sqrt(2 lambda1), lambda1 <= (|T0|^2 + |T1|^2) 1.1 s^2 smax^2 + 0.6 (as in CalcViewGeom's early cull),
// |T0|^2 + |T1|^2 <= (focal / w)^2 G with G = 2 (|mv0|^2 + |mv1|^2 + (limX^2 + limY^2) |mv2|^2)  =>  half extent <=
// K focal smax / w + 3.1 px with K = 2 sqrt(2) sqrt(2.2 G s^2).  "Right of the screen" (cx - extent > W) becomes the LINEAR test
// x - w (1 + 13.2 / W) - (2 K focal / W) smax > 0 on clip coordinates (slack: K is taken 5 % larger, 6.6 px instead of 3.1);
// likewise left / top / bottom; the depth planes are the rasteriser's own centre-depth rule.  Needs clip.w = |view z|
// (a perspective projection whose last row is (0, 0, -1, 0)); the host checks that and switches the cull off otherwise.
GS_HD void FrameConstsChunkCull(FrameConsts& c) {
    const float g0 = dot3f(c.mv[0], c.mv[1], c.mv[2], c.mv[0], c.mv[1], c.mv[2]), g1 = dot3f(c.mv[4], c.mv[5], c.mv[6], c.mv[4], c.mv[5], c.mv[6]);
    const float g2 = dot3f(c.mv[8], c.mv[9], c.mv[10], c.mv[8], c.mv[9], c.mv[10]);
    const float G = 2.0f * (g0 + g1 + (c.limX * c.limX + c.limY * c.limY) * g2);
    const float K = (GS_CULL_EXTENT * 1.05f) * sqrtf(2.2f * G * (c.splatScale * c.splatScale));
    c.cullKx = 2.0f * K * c.focal / c.screenW;
    c.cullKy = 2.0f * K * c.focal / c.screenH;
    c.cullMx = 1.0f + 13.2f / c.screenW;
    c.cullMy = 1.0f + 13.2f / c.screenH;
    // clip.w of a point must equal -(mv row 2).point: compare row 3 of vp * o2w with -row 2 of mv
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
        float r = 0.0f;
        for (int j = 0; j < 3; ++j) r += c.vp[12 + j] * c.o2w[j * 4 + k];
        if (k == 3) r += c.vp[15];
        const float want = -c.mv[8 + k];
        if (!(fabsf(r - want) <= 1.0e-4f * (fabsf(want) + 1.0f))) ok = false;
    }
    if (!(K > 0.0f) || !(K < 3.0e30f)) ok = false;
    c.cullOn = ok ? 1u : 0u;
}

// corner: 0..7 (bit 0 = x max, bit 1 = y max, bit 2 = z max).  planes[p] = this corner is on the outer side of plane p
// (0 right, 1 left, 2 above-or-below +y, 3 the other y side, 4 nearer than near, 5 beyond far).
GS_HD uint32_t ChunkCornerOutside(const AssetView& a, const FrameConsts& P, uint32_t chunkIdx, uint32_t corner) {
    const uint8_t* ck = a.chunk + (uint64_t)chunkIdx * 64;
    const float px = u2f(ld32a(ck, 16 + ((corner & 1u) ? 4 : 0))), py = u2f(ld32a(ck, 24 + ((corner & 2u) ? 4 : 0))), pz = u2f(ld32a(ck, 32 + ((corner & 4u) ? 4 : 0)));
    float sm = fmaxf(fmaxf(f16tof32(ld32a(ck, 40) >> 16), f16tof32(ld32a(ck, 44) >> 16)), f16tof32(ld32a(ck, 48) >> 16));
    sm *= sm; sm *= sm; sm *= sm;                                   // the asset stores scale^(1/8)
    const float wx = mrow(P.o2w, 0, px, py, pz), wy = mrow(P.o2w, 1, px, py, pz), wz = mrow(P.o2w, 2, px, py, pz);
    const float x = mrow(P.vp, 0, wx, wy, wz), y = mrow(P.vp, 1, wx, wy, wz), w = mrow(P.vp, 3, wx, wy, wz);
    const float cxs = P.cullKx * sm, cys = P.cullKy * sm;
    uint32_t m = 0;
    if (x - w * P.cullMx - cxs > 0.0f) m |= 1u;
    if (-x - w * P.cullMx - cxs > 0.0f) m |= 2u;
    if (y - w * P.cullMy - cys > 0.0f) m |= 4u;
    if (-y - w * P.cullMy - cys > 0.0f) m |= 8u;
    if (w < P.nearClip) m |= 16u;
    if (w > P.farClip) m |= 32u;
    return m;
}
GS_HD bool ChunkOutside(const AssetView& a, const FrameConsts& P, uint32_t chunkIdx) {       // scalar form (host tests)
    if (!P.cullOn || chunkIdx >= a.chunkCount) return false;
    uint32_t all = 63u;
    for (uint32_t c = 0; c < 8; ++c) all &= ChunkCornerOutside(a, P, chunkIdx, c);
    return all != 0u;
}


// ---- BC7 (BPTC) block decode: ColorFormat.BC7 = GraphicsFormat.RGBA_BC7_UNorm (GaussianSplatAsset.cs:56,169), the colour
// texture of the VeryLow preset (GaussianSplatAssetCreator.cs:198,893-910), sampled by _SplatColor.Load in LoadSplatData.
// The texture unit decodes the 16-byte block of the 4x4 texels around the splat's texel; here: one block load + the decode
// of that ONE texel.  Format: Khronos Data Format Specification, "BPTC"; the partition / anchor tables are those of
// unitygaussiansplatting_amd/bc7.py, extracted from and cross-checked against an independent decoder (Pillow) by
// tests/test_bc7.py.  Returns r | g << 8 | b << 16 | a << 24.
GS_HD uint32_t bc7_bits(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t n) {      // n <= 8 bits at bit `pos` of the 128-bit block
    uint64_t v;
    if (pos >= 64u) v = hi >> (pos - 64u);
    else v = (lo >> pos) | (pos ? (hi << (64u - pos)) : 0ull);
    return (uint32_t)v & ((1u << n) - 1u);
}
GS_HD uint32_t DecodeBC7Texel(const uint8_t* block, uint32_t texel) {
        static constexpr uint16_t kP2[64] = { 0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000, 0xf710, 0x8e, 0x7100, 0x8ce, 0x8c, 0x7310, 0x3100, 0x8cce, 0x88c, 0x3110, 0x6666, 0x366c, 0x17e8, 0xff0, 0x718e, 0x399c, 0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x660, 0x272, 0x4e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0xfcc, 0x7744, 0xee22 };
        static constexpr uint32_t kP3[64] = { 0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050, 0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250, 0xa5945040, 0xa425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500, 0x50a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200, 0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0xaa5500, 0x24924924, 0x24499224, 0x50a50a50, 0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600, 0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000, 0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254 };
        static constexpr uint8_t kA2[64] = { 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2, 15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 };
        static constexpr uint8_t kA3a[64] = { 3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15, 8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3 };
        static constexpr uint8_t kA3b[64] = { 15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8, 15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8 };
        // per mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits, endpoint p-bits, shared p-bits,
        // index bits, secondary index bits -- packed 4 bits each, lowest nibble first
        static constexpr uint64_t kMode[8] = { 0x301040043ull, 0x310060062ull, 0x200050063ull, 0x201070062ull, 0x3200651201ull, 0x2200870201ull, 0x401770001ull, 0x201550062ull };
        static constexpr uint8_t kW2[4] = { 0, 21, 43, 64 };
        static constexpr uint8_t kW3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 };
        static constexpr uint8_t kW4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };
    const uint64_t lo = (uint64_t)ld32a(block, 0) | ((uint64_t)ld32a(block, 4) << 32), hi = (uint64_t)ld32a(block, 8) | ((uint64_t)ld32a(block, 12) << 32);
    const uint32_t m8 = (uint32_t)lo & 255u;
    if (m8 == 0u) return 0u;                                              // reserved mode: the block decodes to zero
    uint32_t mode = 0;
    while (!((m8 >> mode) & 1u)) ++mode;
    const uint64_t mi = kMode[mode];
    const uint32_t ns = (uint32_t)(mi & 15), pb = (uint32_t)(mi >> 4) & 15, rb = (uint32_t)(mi >> 8) & 15, isb = (uint32_t)(mi >> 12) & 15,
                   cb = (uint32_t)(mi >> 16) & 15, ab = (uint32_t)(mi >> 20) & 15, epb = (uint32_t)(mi >> 24) & 15, spb = (uint32_t)(mi >> 28) & 15,
                   ib = (uint32_t)(mi >> 32) & 15, ib2 = (uint32_t)(mi >> 36) & 15;
    uint32_t pos = mode + 1u;
    const uint32_t shape = bc7_bits(lo, hi, pos, pb); pos += pb;
    const uint32_t rot = bc7_bits(lo, hi, pos, rb); pos += rb;
    const uint32_t isel = bc7_bits(lo, hi, pos, isb); pos += isb;
    uint32_t s = 0, an1 = 16u, an2 = 16u;                                 // subset of the texel, anchors of subsets 1 and 2
    if (ns == 2u) { s = (kP2[shape] >> texel) & 1u; an1 = kA2[shape]; }
    else if (ns == 3u) { s = (kP3[shape] >> (2u * texel)) & 3u; an1 = kA3a[shape]; an2 = kA3b[shape]; }
    const uint32_t ne = 2u * ns, e0 = 2u * s, e1 = e0 + 1u;
    uint32_t c0[4], c1[4];
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        c0[ch] = bc7_bits(lo, hi, pos + (ch * ne + e0) * cb, cb);
        c1[ch] = bc7_bits(lo, hi, pos + (ch * ne + e1) * cb, cb);
    }
    pos += 3u * ne * cb;
    c0[3] = 255u; c1[3] = 255u;
    if (ab) { c0[3] = bc7_bits(lo, hi, pos + e0 * ab, ab); c1[3] = bc7_bits(lo, hi, pos + e1 * ab, ab); pos += ne * ab; }
    uint32_t cbits = cb, abits = ab;
    if (epb) {
        const uint32_t p0 = bc7_bits(lo, hi, pos + e0, 1), p1 = bc7_bits(lo, hi, pos + e1, 1);
        pos += ne;
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ++ch) { c0[ch] = (c0[ch] << 1) | p0; c1[ch] = (c1[ch] << 1) | p1; }
        if (ab) { c0[3] = (c0[3] << 1) | p0; c1[3] = (c1[3] << 1) | p1; abits++; }
        cbits++;
    } else if (spb) {
        const uint32_t p = bc7_bits(lo, hi, pos + s, 1);
        pos += ns;
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ++ch) { c0[ch] = (c0[ch] << 1) | p; c1[ch] = (c1[ch] << 1) | p; }
        cbits++;
    }
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) {                                 // left-align to 8 bits, replicate the top bits
        c0[ch] <<= 8u - cbits; c0[ch] |= c0[ch] >> cbits;
        c1[ch] <<= 8u - cbits; c1[ch] |= c1[ch] >> cbits;
    }
    if (ab) { c0[3] <<= 8u - abits; c0[3] |= c0[3] >> abits; c1[3] <<= 8u - abits; c1[3] |= c1[3] >> abits; }
    // index of this texel: ib bits per texel, one bit less for each subset's anchor texel
    const uint32_t before = (texel > 0u ? 1u : 0u) + (texel > an1 ? 1u : 0u) + (texel > an2 ? 1u : 0u);
    const bool isAnchor = texel == 0u || texel == an1 || texel == an2;
    uint32_t i1 = bc7_bits(lo, hi, pos + texel * ib - before, ib - (isAnchor ? 1u : 0u));
    pos += 16u * ib - ns;
    uint32_t ci = i1, cbt = ib, ai = i1, abt = ib;
    if (ib2) {
        const uint32_t i2 = bc7_bits(lo, hi, pos + texel * ib2 - (texel > 0u ? 1u : 0u), ib2 - (texel == 0u ? 1u : 0u));
        ai = i2; abt = ib2;
        if (isel) { ci = i2; cbt = ib2; ai = i1; abt = ib; }
    }
    const uint32_t wc = cbt == 2u ? kW2[ci] : (cbt == 3u ? kW3[ci] : kW4[ci]);
    const uint32_t wa = abt == 2u ? kW2[ai] : (abt == 3u ? kW3[ai] : kW4[ai]);
    uint32_t px[4];
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) px[ch] = ((64u - wc) * c0[ch] + wc * c1[ch] + 32u) >> 6;
    px[3] = ((64u - wa) * c0[3] + wa * c1[3] + 32u) >> 6;
    if (rot == 1u) { const uint32_t t = px[3]; px[3] = px[0]; px[0] = t; }
    else if (rot == 2u) { const uint32_t t = px[3]; px[3] = px[1]; px[1] = t; }
    else if (rot == 3u) { const uint32_t t = px[3]; px[3] = px[2]; px[2] = t; }
    return px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
}

// _SplatColor.Load(SplatIndexToPixelIndex(idx)) (GaussianSplatting.hlsl:456-458): the texel as the texture unit returns it,
// before the chunk de-normalisation
template <class F = RuntimeFormats> GS_HD V4 LoadColorTexel(const AssetView& a, uint32_t idx) {
    uint32_t tx, ty;
    SplatIndexToPixelIndex(idx, tx, ty);
    const uint64_t texel = (uint64_t)ty * 2048 + tx;
    const uint32_t colorFmt = F::colorFmt(a);
    if (colorFmt == 0) {
        const uint8_t* c = a.color + texel * 16;
        return { u2f(ld32a(c, 0)), u2f(ld32a(c, 4)), u2f(ld32a(c, 8)), u2f(ld32a(c, 12)) };
    }
    if (colorFmt == 1) {
        const uint32_t lo = ld32a(a.color, texel * 8), hi = ld32a(a.color, texel * 8 + 4);
        return { f16tof32(lo), f16tof32(lo >> 16), f16tof32(hi), f16tof32(hi >> 16) };
    }
    uint32_t e;
    if (colorFmt == 3) e = DecodeBC7Texel(a.color + ((uint64_t)(ty >> 2) * 512 + (tx >> 2)) * 16, (ty & 3u) * 4u + (tx & 3u));   // RGBA_BC7_UNorm, 512 blocks per row
    else e = ld32a(a.color, texel * 4);
    return { (float)(e & 255) * GS_R255, (float)((e >> 8) & 255) * GS_R255, (float)((e >> 16) & 255) * GS_R255, (float)(e >> 24) * GS_R255 };
}

// splat.sh.col of LoadSplatData: the de-normalised DC colour (GaussianSplatting.hlsl:456-458,590-596), what the debug point
// shader shows (GaussianDebugRenderPoints.shader:48)
GS_HD V3 LoadSplatBaseColor(const AssetView& a, uint32_t idx) {
    V4 col = LoadColorTexel(a, idx);
    const uint32_t ci = idx >> 8;
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        col.x = lerpf(f16tof32(ld32a(c, 0)), f16tof32(ld32a(c, 0) >> 16), col.x);
        col.y = lerpf(f16tof32(ld32a(c, 4)), f16tof32(ld32a(c, 4) >> 16), col.y);
        col.z = lerpf(f16tof32(ld32a(c, 8)), f16tof32(ld32a(c, 8) >> 16), col.z);
    }
    return { col.x, col.y, col.z };
}
// GaussianDebugRenderPoints.shader:49-54 (_DisplayIndex): a colour that encodes the splat's index
GS_HD V3 DebugIndexColor(uint32_t idx, uint32_t count) {
    const float f = (float)idx / (float)count;
    const float r = f * 100.0f, g = f * 10.0f;
    return { r - floorf(r), g - floorf(g), f };
}

// ---- debug box modes (GaussianDebugRenderBoxes.shader): every box is an affine image of the cube [-1,1]^3,
// world = c + B l.  Per pixel the rasteriser's result is restated as a ray / box intersection in the box's own space
// (l = Binv (p - c)): the ray through the pixel centre is p(t) = o + t d with d scaled so that t IS the view depth, the slab
// test gives its entry / exit parameters, and the face the rasteriser draws is the entry face for a box whose transform
// keeps the winding (the cube's triangles are wound so that its outside faces are the back faces: with `Cull Front` the
// faces turned towards the camera are drawn) and the exit face for a mirrored one.  Depth clipping and the depth test use t.
struct BoxRec { float inv[9]; float lo[3]; float r, g, b, a; };      // 64 B: Binv rows, Binv (o - c), colour; a < 0 marks a mirrored box (its alpha is |a|)

// inverse of a 3x3 (rows of 3) by cofactors; returns the determinant.  A singular / non-finite box is not drawn.
GS_HD float Inverse3(const float* b, float* inv) {
    const float c00 = fmaf(b[4], b[8], -(b[5] * b[7])), c01 = fmaf(b[5], b[6], -(b[3] * b[8])), c02 = fmaf(b[3], b[7], -(b[4] * b[6]));
    const float det = fmaf(b[2], c02, fmaf(b[1], c01, b[0] * c00));
    const float r = 1.0f / det;
    inv[0] = c00 * r; inv[1] = fmaf(b[2], b[7], -(b[1] * b[8])) * r; inv[2] = fmaf(b[1], b[5], -(b[2] * b[4])) * r;
    inv[3] = c01 * r; inv[4] = fmaf(b[0], b[8], -(b[2] * b[6])) * r; inv[5] = fmaf(b[2], b[3], -(b[0] * b[5])) * r;
    inv[6] = c02 * r; inv[7] = fmaf(b[1], b[6], -(b[0] * b[7])) * r; inv[8] = fmaf(b[0], b[4], -(b[1] * b[3])) * r;
    return det;
}

// per-frame ray set-up from the frame constants: R0 = VP row 0 / P00, R1 = VP row 1 / P11 (the camera's right / up axes in
// world space), R2 = VP row 3 (its forward axis: clip.w = view depth).  World direction of the ray through pixel centre
// (px + 0.5, py + 0.5): d = ax R0 + ay R1 + R2, ax = ndc.x / P00, ay = ndc.y / P11 -- so that view depth along the ray = t.
struct RayConsts { float r0[3], r1[3], r2[3]; float ox, oy, oz; float p00, p11, W, H; };
GS_HD void RayConstsFromFrame(RayConsts& rc, const float* vp, float p00, float p11, float camx, float camy, float camz, float W, float H) {
    for (int k = 0; k < 3; ++k) { rc.r0[k] = vp[k] / p00; rc.r1[k] = vp[4 + k] / p11; rc.r2[k] = vp[12 + k]; }
    rc.ox = camx; rc.oy = camy; rc.oz = camz; rc.p00 = p00; rc.p11 = p11; rc.W = W; rc.H = H;
}
GS_HD void PixelRay(const RayConsts& rc, int px, int py, float d[3]) {
    const float ndcx = (((float)px + 0.5f) / rc.W) * 2.0f - 1.0f;
    const float ndcy = 1.0f - (((float)py + 0.5f) / rc.H) * 2.0f;
    const float ax = ndcx / rc.p00, ay = ndcy / rc.p11;
    for (int k = 0; k < 3; ++k) d[k] = fmaf(ay, rc.r1[k], fmaf(ax, rc.r0[k], rc.r2[k]));
}
// view depth of the drawn face of box `inv/lo` along the ray with box-space direction ld, or a negative value if the pixel is
// not covered.  NaNs (a ray parallel to a slab it starts on) compare false: not covered.
GS_HD float BoxFaceDepth(const float* lo, const float* ld, bool mirrored) {
    float tmin = -3.4028234663852886e38f, tmax = 3.4028234663852886e38f;
    for (int k = 0; k < 3; ++k) {
        const float t1 = (-1.0f - lo[k]) / ld[k], t2 = (1.0f - lo[k]) / ld[k];
        tmin = fmaxf(tmin, fminf(t1, t2));
        tmax = fminf(tmax, fmaxf(t1, t2));
    }
    if (!(tmin <= tmax)) return -1.0f;
    const float t = mirrored ? tmax : tmin;
    return (t > 0.0f) ? t : -1.0f;
}

// LoadSplatData's rotation, scale (de-normalised) and opacity (GaussianSplatting.hlsl:428-470,565-603) for the box mode
GS_HD void LoadSplatRotScaleOpacity(const AssetView& a, uint32_t idx, V4& q, V3& scale, float& opacity) {
    uint32_t otherStride = 4 + vecStride(a.scaleFmt);
    if (a.shFmt > 3) otherStride += 2;
    const uint64_t otherAddr = (uint64_t)idx * otherStride;
    q = DecodeRotation(LoadUInt(a.other, otherAddr));
    scale = LoadVec(a.other, otherAddr + 4, a.scaleFmt);
    V4 col = LoadColorTexel(a, idx);
    const uint32_t ci = idx >> 8;
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        scale.x = lerpf(f16tof32(ld32a(c, 40)), f16tof32(ld32a(c, 40) >> 16), scale.x);
        scale.y = lerpf(f16tof32(ld32a(c, 44)), f16tof32(ld32a(c, 44) >> 16), scale.y);
        scale.z = lerpf(f16tof32(ld32a(c, 48)), f16tof32(ld32a(c, 48) >> 16), scale.z);
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        col.w = InvSquareCentered01(lerpf(f16tof32(ld32a(c, 12)), f16tof32(ld32a(c, 12) >> 16), col.w));
    }
    opacity = col.w;
}

// Builds the record of one box from its centre c and matrix B (world = c + B l, rows of 3); returns false if it cannot be drawn.
// Also the conservative pixel bounding box of its projection (the whole screen if a corner is not in front of the camera).
GS_HD bool BuildBox(const float c[3], const float B[9], const RayConsts& rc, const float* vp, float r, float g, float bl, float al,
                    BoxRec& rec, int& x0, int& x1, int& y0, int& y1) {
    const float det = Inverse3(B, rec.inv);
    bool ok = finite32(det) && det != 0.0f;
    for (int k = 0; k < 9; ++k) ok = ok && finite32(rec.inv[k]);
    if (!ok || !(al > 0.0f)) return false;
    const float dx = rc.ox - c[0], dy = rc.oy - c[1], dz = rc.oz - c[2];
    for (int k = 0; k < 3; ++k) rec.lo[k] = fmaf(rec.inv[k * 3 + 2], dz, fmaf(rec.inv[k * 3 + 1], dy, rec.inv[k * 3] * dx));
    rec.r = r; rec.g = g; rec.b = bl; rec.a = det < 0.0f ? -al : al;
    float minx = 3.0e38f, maxx = -3.0e38f, miny = 3.0e38f, maxy = -3.0e38f;
    bool behind = false;
    for (int corner = 0; corner < 8; ++corner) {
        const float lx = (corner & 1) ? 1.0f : -1.0f, ly = (corner & 2) ? 1.0f : -1.0f, lz = (corner & 4) ? 1.0f : -1.0f;
        const float wx = c[0] + fmaf(B[2], lz, fmaf(B[1], ly, B[0] * lx)), wy = c[1] + fmaf(B[5], lz, fmaf(B[4], ly, B[3] * lx)),
                    wz = c[2] + fmaf(B[8], lz, fmaf(B[7], ly, B[6] * lx));
        const float cx = mrow(vp, 0, wx, wy, wz), cy = mrow(vp, 1, wx, wy, wz), cw = mrow(vp, 3, wx, wy, wz);
        if (!(cw > 1.0e-6f)) { behind = true; continue; }
        const float sx = fmaf(0.5f * (cx / cw), rc.W, 0.5f * rc.W), sy = fmaf(-0.5f * (cy / cw), rc.H, 0.5f * rc.H);
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx); miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
    if (behind || !(finite32(minx) && finite32(maxx) && finite32(miny) && finite32(maxy))) { x0 = 0; y0 = 0; x1 = (int)rc.W - 1; y1 = (int)rc.H - 1; return true; }
    const float fx0 = fmaxf(floorf(minx) - 1.0f, 0.0f), fx1 = fminf(ceilf(maxx) + 1.0f, rc.W - 1.0f);
    const float fy0 = fmaxf(floorf(miny) - 1.0f, 0.0f), fy1 = fminf(ceilf(maxy) + 1.0f, rc.H - 1.0f);
    if (!(fx0 <= fx1 && fy0 <= fy1)) return false;
    x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1;
    return true;
}

// IsSplatCut (SplatUtilities.compute:164-187); pos is the object-space position
GS_HD bool IsSplatCut(const EditView& e, float px, float py, float pz) {
    bool finalCut = false;
    for (uint32_t i = 0; i < e.cutoutCount; ++i) {
        const uint32_t* c = e.cutouts + i * 17u;                   // wave-uniform address: scalar loads
        const uint32_t tf = c[16];
        const uint32_t type = tf & 0xFFu;
        if (type == 0xFFu) continue;                               // invalid/null cutout, ignore
        const bool invert = (tf & 0xFF00u) != 0;
        float m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = u2f(c[k]);
        const float cx = mrow(m, 0, px, py, pz), cy = mrow(m, 1, px, py, pz), cz = mrow(m, 2, px, py, pz);
        if (type == 0u) { if (dot3f(cx, cy, cz, cx, cy, cz) <= 1.0f) return invert; }
        if (type == 1u) { if (fabsf(cx) <= 1.0f && fabsf(cy) <= 1.0f && fabsf(cz) <= 1.0f) return invert; }
        finalCut = finalCut || !invert;
    }
    return finalCut;
}

// ---- the edit kernels' per-splat arithmetic (SplatUtilities.compute:266-423; kernels in gs_edit.hip) ----
// What CSSelectionUpdate reads of a frame: _MatrixObjectToWorld (rows 0..2), UNITY_MATRIX_VP, _VecScreenParams.xy and
// _SelectionRect = (x_min, y_min, x_max, y_max) in pixels, y up from the bottom edge
struct EditSelect {
    float o2w[12];
    float vp[16];
    float screenW, screenH;
    float rect[4];
};

// gs_renderer_edit_select_surface: the inclusive pixel rectangle clipped to the target (w = 0: nothing left), the renderer's tag and the operation
struct PickSelect {
    uint32_t x0, y0, w, h;          // clipped rectangle, pixels
    uint32_t stride;                // the target's width: records per row
    uint32_t tag;
    uint32_t subtract;
};

// CSSelectionUpdate's test of one splat (SplatUtilities.compute:400-416): does the rectangle select it?  World and clip position
// are CalcViewGeom's expressions, so the clip position has the bits of the view record's pos.  Every comparison is the
// reference's, literally: a NaN w is not "behind", and a NaN pixel position is outside no edge of the rectangle, so it is a hit.
// the part of the test that both screen tools share: false = cut or behind the camera, else the pixel position (y up from the bottom edge)
GS_HD bool EditSelectionPixel(const EditSelect& S, const EditView& E, const V3& pos, float& px, float& py) {
    if (IsSplatCut(E, pos.x, pos.y, pos.z)) return false;
    const float wx = mrow(S.o2w, 0, pos.x, pos.y, pos.z), wy = mrow(S.o2w, 1, pos.x, pos.y, pos.z), wz = mrow(S.o2w, 2, pos.x, pos.y, pos.z);
    const float cx = mrow(S.vp, 0, wx, wy, wz), cy = mrow(S.vp, 1, wx, wy, wz), cw = mrow(S.vp, 3, wx, wy, wz);
    if (cw <= 0.0f) return false;                                  // behindCam
    px = ((cx / cw) * 0.5f + 0.5f) * S.screenW;                    // (centerClipPos.y *= -1 first, :406)
    py = (((-cy) / cw) * -0.5f + 0.5f) * S.screenH;
    return true;
}
GS_HD bool EditSelectionHit(const EditSelect& S, const EditView& E, const V3& pos) {
    float px, py;
    if (!EditSelectionPixel(S, E, pos, px, py)) return false;
    if (px < S.rect[0] || px > S.rect[2] || py < S.rect[1] || py > S.rect[3]) return false;
    return true;
}

// ---- the screen mask (gs_mask; kernels in gs_mask.hip and gs_edit.hip) ----
// One bit per pixel of a W x H screen, row 0 = top: a row is ceil(W/32) words, bit x & 31 of word x >> 5 is pixel x, the bits beyond W are zero.
// Everything below is fp32 and rounds once per operation; the centre of pixel (x, y) is ((float)x + 0.5f, (float)y + 0.5f), exact for x, y < 65536.
constexpr float kMaskCoordMax = 65536.0f;                          // |coordinate| and radius limit of the drawing calls
constexpr uint32_t kMaskMaxPoints = 65536u;
struct MaskView { const uint32_t* words; uint32_t w, h, rowWords; };
GS_HD uint32_t MaskRowWords(uint32_t w) { return (w + 31u) >> 5; }
GS_HD uint32_t MaskTailBits(uint32_t w) { return (w & 31u) ? (1u << (w & 31u)) - 1u : 0xFFFFFFFFu; }    // the valid bits of a row's last word
GS_HD bool MaskCoordOk(float v) { return fabsf(v) <= kMaskCoordMax; }                                    // false for NaN and the infinities
GS_HD bool MaskBit(const MaskView& M, uint32_t x, uint32_t y) { return ((M.words[(size_t)y * M.rowWords + (x >> 5)] >> (x & 31u)) & 1u) != 0u; }

// the lasso counterpart of the rectangle comparison: px, py as EditSelectionPixel leaves them (py up from the bottom edge).  A NaN fails every comparison.
GS_HD bool MaskPixelHit(const MaskView& M, float px, float py) {
    if (!(px >= 0.0f && px < (float)M.w && py >= 0.0f && py < (float)M.h)) return false;
    return MaskBit(M, (uint32_t)px, M.h - 1u - (uint32_t)py);
}
GS_HD bool EditSelectionMaskHit(const EditSelect& S, const EditView& E, const MaskView& M, const V3& pos) {
    float px, py;
    if (!EditSelectionPixel(S, E, pos, px, py)) return false;
    return MaskPixelHit(M, px, py);
}

// polygon, even-odd: on the row with centre yc an edge (a -> b) crosses iff exactly one end is at or above the centre line ...
GS_HD bool MaskEdgeCrosses(float ay, float by, float yc) { return (ay <= yc) != (by <= yc); }
// ... at this abscissa (by != ay for a crossing edge, and |yc - ay| <= |by - ay|: finite under the coordinate limit), and toggles every pixel with xc < xs
GS_HD float MaskEdgeCrossX(float ax, float ay, float bx, float by, float yc) { return ax + ((yc - ay) * (bx - ax)) / (by - ay); }
// k = the number of pixels x in [0, W) with (float)x + 0.5f < xs, for EVERY float xs.  The predicate is monotone in x, so the toggled pixels are 0 .. k-1.
//   not (xs > 0.5): no pixel (x + 0.5 >= 0.5 >= xs; a NaN compares false everywhere).   xs >= W: all of them (x + 0.5 <= W - 0.5 < xs).
//   else f = floor(xs) is an integer in [0, W), exact: pixels x < f have x + 0.5 <= f - 0.5 < xs, pixels x > f have x + 0.5 >= f + 1.5 > xs, and
//   pixel f is decided by the comparison itself, f + 0.5 being exact below 2^23.
GS_HD uint32_t MaskBoundaryCount(float xs, uint32_t w) {
    if (!(xs > 0.5f)) return 0u;
    if (xs >= (float)w) return w;
    const float f = floorf(xs);
    return (uint32_t)f + ((f + 0.5f < xs) ? 1u : 0u);
}

// stroke: is the pixel centre (cx, cy) within `r2 = radius * radius` of the segment (a -> b)?  a == b is a disc
GS_HD bool MaskSegmentCovers(float ax, float ay, float bx, float by, float cx, float cy, float r2) {
    const float dx = bx - ax, dy = by - ay, ex = cx - ax, ey = cy - ay;
    const float len2 = dx * dx + dy * dy;
    float t = 0.0f;
    if (len2 != 0.0f) t = fminf(fmaxf((ex * dx + ey * dy) / len2, 0.0f), 1.0f);
    const float tx = t * dx, ty = t * dy;
    const float qx = ex - tx, qy = ey - ty;
    const float d2 = qx * qx + qy * qy;
    return d2 <= r2;
}
// The conservative pixel box of a segment, clipped to the screen: every pixel MaskSegmentCovers accepts lies in [x0, x1] x [y0, y1] (x0 > x1 or y0 > y1:
// none on screen).  R = radius + 1: a covered centre is within radius + 2^-4 of the true segment (DESIGN.md section 4.20 has the rounding argument), and
// the box's own three roundings move an edge by less than 2^-5.  Pixel x can only be covered if lo <= x + 0.5 <= hi, so x in [floor(lo), floor(hi)].
struct MaskBox { int32_t x0, y0, x1, y1; };
GS_HD MaskBox MaskSegmentBox(float ax, float ay, float bx, float by, float radius, uint32_t w, uint32_t h) {
    const float R = radius + 1.0f;
    const float lox = fminf(ax, bx) - R, hix = fmaxf(ax, bx) + R, loy = fminf(ay, by) - R, hiy = fmaxf(ay, by) + R;
    MaskBox B;
    B.x0 = (int32_t)fmaxf(floorf(lox), 0.0f); B.x1 = (int32_t)fminf(floorf(hix), (float)w - 1.0f);
    B.y0 = (int32_t)fmaxf(floorf(loy), 0.0f); B.y1 = (int32_t)fminf(floorf(hiy), (float)h - 1.0f);
    return B;
}

// CSUpdateEditData's bounds of one selected splat (SplatUtilities.compute:279-296), as the sortable uints the kernel's
// InterlockedMin / Max take: min(1e38, p) / max(-1e38, p) per component -- fminf / fmaxf drop a NaN as HLSL's min / max do.
// FloatToSortableUint is monotonic over every float, so integer min / max of these in any grouping gives the same bits.
GS_HD void EditSplatBounds(const V3& pos, uint32_t lo[3], uint32_t hi[3]) {
    lo[0] = FloatToSortableUint(fminf(1.0e38f, pos.x)); hi[0] = FloatToSortableUint(fmaxf(-1.0e38f, pos.x));
    lo[1] = FloatToSortableUint(fminf(1.0e38f, pos.y)); hi[1] = FloatToSortableUint(fmaxf(-1.0e38f, pos.y));
    lo[2] = FloatToSortableUint(fminf(1.0e38f, pos.z)); hi[2] = FloatToSortableUint(fmaxf(-1.0e38f, pos.z));
}

// CSTranslateSelection / CSRotateSelection / CSScaleSelection for one selected splat (SplatUtilities.compute:425-521).  What the three
// read of their dispatch: _SelectionCenter, _MatrixObjectToWorld and _MatrixWorldToObject (rows 0..2), and _SelectionDelta (xyz; translate,
// scale) or _SelectionDeltaRot (xyzw; rotate).  mul(M, float4(p, 1)) is mrow's fmaf chain, as everywhere; every other operation rounds once,
// in the order of the reference's text.  SHs are not rotated and a splat's own scale is not scaled: the reference's @TODOs, kept unless the
// renderer's rigid-transform setting is on (EditRigid*, below BakeSplatTransform).
struct EditXform { float center[3]; float o2w[12]; float w2o[12]; float delta[4]; };
GS_HD V3 EditTranslatePos(const EditXform& X, const V3& pos) { return { pos.x + X.delta[0], pos.y + X.delta[1], pos.z + X.delta[2] }; }
GS_HD V3 EditRotatePos(const EditXform& X, const V3& mouseDown) {
    V3 p = { mouseDown.x - X.center[0], mouseDown.y - X.center[1], mouseDown.z - X.center[2] };
    p = { mrow(X.o2w, 0, p.x, p.y, p.z), mrow(X.o2w, 1, p.x, p.y, p.z), mrow(X.o2w, 2, p.x, p.y, p.z) };
    p = QuatRotateVector(p, { X.delta[0], X.delta[1], X.delta[2], X.delta[3] });
    p = { mrow(X.w2o, 0, p.x, p.y, p.z), mrow(X.w2o, 1, p.x, p.y, p.z), mrow(X.w2o, 2, p.x, p.y, p.z) };
    return { p.x + X.center[0], p.y + X.center[1], p.z + X.center[2] };
}
GS_HD V3 EditScalePos(const EditXform& X, const V3& mouseDown) {
    V3 p = { mouseDown.x - X.center[0], mouseDown.y - X.center[1], mouseDown.z - X.center[2] };
    p = { mrow(X.o2w, 0, p.x, p.y, p.z), mrow(X.o2w, 1, p.x, p.y, p.z), mrow(X.o2w, 2, p.x, p.y, p.z) };
    p = { p.x * X.delta[0], p.y * X.delta[1], p.z * X.delta[2] };
    p = { mrow(X.w2o, 0, p.x, p.y, p.z), mrow(X.w2o, 1, p.x, p.y, p.z), mrow(X.w2o, 2, p.x, p.y, p.z) };
    return { p.x + X.center[0], p.y + X.center[1], p.z + X.center[2] };
}
// the rotation word of a rotated splat: decode the mouse-down word, QuatMul(rot, delta) ("@TODO: correct rotation": the reference's), encode
GS_HD uint32_t EditRotateWord(const EditXform& X, uint32_t mouseDown) {
    return EncodeQuatToNorm10(PackSmallest3Rotation(QuatMul(DecodeRotation(mouseDown), { X.delta[0], X.delta[1], X.delta[2], X.delta[3] })));
}

// CSCalcViewData for one splat (SplatUtilities.compute:189-252), in two halves so that a caller which only needs the
// splats that reach the screen can stop after the geometry:
//   CalcViewGeom   LoadSplatData minus SH, clip position, deleted bit / cutouts, 3D -> 2D covariance, axes, opacity
//   CalcViewColor  view direction, ShadeSH, colour packing
// CalcViewDataT = both, i.e. the reference's kernel; the arithmetic is the same whichever way it is called.
struct ViewPartial {
    ViewData view;              // pos, axis1/2 final after CalcViewGeom; color[1] low half = f16 opacity
    V4 col;                     // de-normalised colour (col.w = opacity before _SplatOpacityScale)
    V3 shMin, shMax;
    float wx, wy, wz;           // centerWorldPos
    uint64_t otherEnd;          // byte address one past the splat's `other` record (the u16 SH index sits just before it)
    bool shLerp;
    bool front;                 // clip.w > 0 after deletion / cutouts: the rest of the record is meaningful
    bool culled;                // allowCull only: the splat cannot reach the screen and the geometry was not finished
};

// outputsOnlyIfDrawn: the caller reads vp (beyond front / culled) only for a splat that passes PrepareSplat -- the per-frame kernel --
// so the record is not zero-filled first (a dozen register moves at every divergent exit of a VALU-bound kernel).
template <class F = RuntimeFormats>
GS_HD void CalcViewGeom(const AssetView& a, const FrameConsts& P, const EditView& E, uint32_t idx, ViewPartial& vp, bool allowCull = false,
                        bool outputsOnlyIfDrawn = false) {
    ViewData& view = vp.view;
    if (!outputsOnlyIfDrawn) {
        view.pos[0] = view.pos[1] = view.pos[2] = view.pos[3] = 0.0f;
        view.axis1[0] = view.axis1[1] = view.axis2[0] = view.axis2[1] = 0.0f;
        view.color[0] = view.color[1] = 0u;
        vp.shLerp = false; vp.otherEnd = 0u;
        vp.shMin = { 0, 0, 0 }; vp.shMax = { 0, 0, 0 }; vp.col = { 0, 0, 0, 0 };
    }
    vp.front = false; vp.culled = false;

    // ---- LoadSplatData: position first (needed for the early out)
    V3 pos = LoadVec(a.pos, (uint64_t)idx * vecStride(F::posFmt(a)), F::posFmt(a));
    const uint32_t ci = idx >> 8;
    const bool chunked = F::chunked(a, ci);
    ChunkRaw ck;
    if (chunked) {
        ck = LoadChunk(a.chunk, ci);
        pos.x = lerpf(u2f(ck.w[4]), u2f(ck.w[5]), pos.x);
        pos.y = lerpf(u2f(ck.w[6]), u2f(ck.w[7]), pos.y);
        pos.z = lerpf(u2f(ck.w[8]), u2f(ck.w[9]), pos.z);
    }
    const float wx = mrow(P.o2w, 0, pos.x, pos.y, pos.z), wy = mrow(P.o2w, 1, pos.x, pos.y, pos.z), wz = mrow(P.o2w, 2, pos.x, pos.y, pos.z);
    vp.wx = wx; vp.wy = wy; vp.wz = wz;
    view.pos[0] = mrow(P.vp, 0, wx, wy, wz);
    view.pos[1] = mrow(P.vp, 1, wx, wy, wz);
    view.pos[2] = mrow(P.vp, 2, wx, wy, wz);
    view.pos[3] = mrow(P.vp, 3, wx, wy, wz);
    // deleted? (:204-214) / cutouts (:216-220): centerClipPos.w = 0, the rest of the clip position is kept
    if (E.deletedBits && ((E.deletedBits[idx >> 5] >> (idx & 31u)) & 1u)) view.pos[3] = 0.0f;
    if (E.cutoutCount && IsSplatCut(E, pos.x, pos.y, pos.z)) view.pos[3] = 0.0f;
    if (view.pos[3] <= 0.0f) return;                               // behindCam (:223), literally: a NaN w is not "behind" (it is never drawn: PrepareSplat)
    vp.front = true;

    // ---- scale (needed first: the early cull below bounds the footprint with it)
    uint32_t otherStride = 4 + vecStride(F::scaleFmt(a));
    if (F::shFmt(a) > 3) otherStride += 2;
    const uint64_t otherAddr = (uint64_t)idx * otherStride;
    vp.otherEnd = otherAddr + otherStride;
    V3 scale = LoadVec(a.other, otherAddr + 4, F::scaleFmt(a));
    if (chunked) {
        scale.x = lerpf(f16tof32(ck.w[10]), f16tof32(ck.w[10] >> 16), scale.x);
        scale.y = lerpf(f16tof32(ck.w[11]), f16tof32(ck.w[11] >> 16), scale.y);
        scale.z = lerpf(f16tof32(ck.w[12]), f16tof32(ck.w[12] >> 16), scale.z);
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
    }
    const float ss2 = P.splatScale * P.splatScale;

    // ---- CalcCovariance2D, first half: the 2x3 matrix T = J * W
    float vx = mrow(P.mv, 0, pos.x, pos.y, pos.z), vy = mrow(P.mv, 1, pos.x, pos.y, pos.z);
    const float vz = mrow(P.mv, 2, pos.x, pos.y, pos.z);
    const float limX = P.limX, limY = P.limY, focal = P.focal;
    // the four divisions by viewPos.z and the two by its square share ONE reciprocal: rz = 1 / z, 1 / z^2 = rz * rz -- what a
    // shader compiler makes of them, and bit for bit what oracle/_ref's fused build of the reference text computes
    const float rz = 1.0f / vz;
    vx = fminf(fmaxf(vx * rz, -limX), limX) * vz;
    vy = fminf(fmaxf(vy * rz, -limY), limY) * vz;
    const float rzz = rz * rz;
    const float J00 = focal * rz, J02 = -(focal * vx) * rzz;
    const float J11 = J00, J12 = -(focal * vy) * rzz;
    const float T00 = fmaf(J02, P.mv[8], J00 * P.mv[0]), T01 = fmaf(J02, P.mv[9], J00 * P.mv[1]), T02 = fmaf(J02, P.mv[10], J00 * P.mv[2]);
    const float T10 = fmaf(J12, P.mv[8], J11 * P.mv[4]), T11 = fmaf(J12, P.mv[9], J11 * P.mv[5]), T12 = fmaf(J12, P.mv[10], J11 * P.mv[6]);

    // ---- early cull (only for callers that do not need the record of a splat that cannot be drawn).  Exactly as
    // PrepareSplat: centre depth outside [near, far] => clipped.  Conservatively: the quad's half extent along x is
    // 2 (|axis1.x| + |axis2.x|) <= 2 sqrt(2) sqrt(axis1.x^2 + axis2.x^2) (Cauchy-Schwarz) <= 2 sqrt(2) sqrt(2 lambda1) (the axes are
    // orthogonal, |axis_k|^2 = 2 lambda_k <= 2 lambda1), the same along y, and lambda1 <= trace(cov2d) <= (|T0|^2 + |T1|^2) lambda_max(Sigma) + 0.6 with
    // lambda_max(Sigma) <= splatScale^2 |R|^2 max(scale)^2  (|R|^2 <= 1.1 for a 10.10.10.2 quaternion); a centre farther than
    // that (+5 %, + 2 px) outside the screen cannot put a fragment on it.  NaNs compare false and take the full path.
    if (allowCull) {
        const float w = view.pos[3];
        if (!(w >= P.nearClip && w <= P.farClip)) { vp.culled = true; return; }
        const float smax = fmaxf(fmaxf(fabsf(scale.x), fabsf(scale.y)), fabsf(scale.z));
        const float t2 = dot3f(T00, T01, T02, T00, T01, T02) + dot3f(T10, T11, T12, T10, T11, T12);
        const float lam = fmaf(t2 * (1.1f * ss2), smax * smax, 0.6f);
        // (a bound with 5 % + 2 px of slack: the GPU's 1-ulp v_sqrt_f32 does, without the ~10-instruction correctly-rounded fix-up)
#if defined(__HIP_DEVICE_COMPILE__)
        const float rad = fmaf(GS_CULL_EXTENT * 1.05f, __builtin_amdgcn_sqrtf(2.0f * lam), 2.0f);
#else
        const float rad = fmaf(GS_CULL_EXTENT * 1.05f, sqrtf(2.0f * lam), 2.0f);
#endif
        const float invw = 1.0f / w;
        const float cx = fmaf(0.5f * (view.pos[0] * invw), P.screenW, 0.5f * P.screenW);
        const float cy = fmaf(-0.5f * (view.pos[1] * invw), P.screenH, 0.5f * P.screenH);
        if (cx - rad > P.screenW || cx + rad < 0.0f || cy - rad > P.screenH || cy + rad < 0.0f) { vp.culled = true; return; }
    }

    // ---- rotation
    const V4 q = DecodeRotation(LoadUInt(a.other, otherAddr));

    // ---- colour texel
    V4 col = LoadColorTexel<F>(a, idx);

    if (chunked) {
        col.x = lerpf(f16tof32(ck.w[0]), f16tof32(ck.w[0] >> 16), col.x);
        col.y = lerpf(f16tof32(ck.w[1]), f16tof32(ck.w[1] >> 16), col.y);
        col.z = lerpf(f16tof32(ck.w[2]), f16tof32(ck.w[2] >> 16), col.z);
        col.w = lerpf(f16tof32(ck.w[3]), f16tof32(ck.w[3] >> 16), col.w);
        col.w = InvSquareCentered01(col.w);
        vp.shMin = { f16tof32(ck.w[13]), f16tof32(ck.w[14]), f16tof32(ck.w[15]) };
        vp.shMax = { f16tof32(ck.w[13] >> 16), f16tof32(ck.w[14] >> 16), f16tof32(ck.w[15] >> 16) };
        vp.shLerp = F::shFmt(a) > 0 && F::shFmt(a) <= 3;
    } else {
        // a chunk-less asset (VeryHigh fp32, or a lossy-format asset created without a chunk blob): CalcViewColor reads these
        // whatever the record's zero-fill above did (outputsOnlyIfDrawn skips it)
        vp.shLerp = false; vp.shMin = { 0, 0, 0 }; vp.shMax = { 0, 0, 0 };
    }
    vp.col = col;

    // ---- CalcMatrixFromRotationScale + CalcCovariance3D
    const float x = q.x, y = q.y, z = q.z, w = q.w;
    // contraction of the nine entries = oracle/_ref's fused build (g++ -ffp-contract=fast of GaussianSplatting.hlsl:40-44): the
    // first product of every sum / difference is the fused one; x*x takes the fusion in r11 and r22, which leaves r00's sum plain
    const float r00 = fmaf(-2.0f, y * y + z * z, 1.0f), r01 = 2.0f * fmaf(x, y, -(w * z)), r02 = 2.0f * fmaf(x, z, w * y);
    const float r10 = 2.0f * fmaf(x, y, w * z), r11 = fmaf(-2.0f, fmaf(x, x, z * z), 1.0f), r12 = 2.0f * fmaf(y, z, -(w * x));
    const float r20 = 2.0f * fmaf(x, z, -(w * y)), r21 = 2.0f * fmaf(y, z, w * x), r22 = fmaf(-2.0f, fmaf(x, x, y * y), 1.0f);
    const float m00 = r00 * scale.x, m01 = r01 * scale.y, m02 = r02 * scale.z;
    const float m10 = r10 * scale.x, m11 = r11 * scale.y, m12 = r12 * scale.z;
    const float m20 = r20 * scale.x, m21 = r21 * scale.y, m22 = r22 * scale.z;
    const float c00 = dot3f(m00, m01, m02, m00, m01, m02) * ss2, c01 = dot3f(m00, m01, m02, m10, m11, m12) * ss2, c02 = dot3f(m00, m01, m02, m20, m21, m22) * ss2;
    const float c11 = dot3f(m10, m11, m12, m10, m11, m12) * ss2, c12 = dot3f(m10, m11, m12, m20, m21, m22) * ss2, c22 = dot3f(m20, m21, m22, m20, m21, m22) * ss2;

    // ---- CalcCovariance2D, second half: cov = T * Sigma * T^T (+ the 0.3 px low-pass)
    // VT[i][j] = sum_k V[i][k] * T[j][k]
    const float VT00 = dot3f(c00, c01, c02, T00, T01, T02), VT01 = dot3f(c00, c01, c02, T10, T11, T12);
    const float VT10 = dot3f(c01, c11, c12, T00, T01, T02), VT11 = dot3f(c01, c11, c12, T10, T11, T12);
    const float VT20 = dot3f(c02, c12, c22, T00, T01, T02), VT21 = dot3f(c02, c12, c22, T10, T11, T12);
    const float cov00 = dot3f(T00, T01, T02, VT00, VT10, VT20) + 0.3f;
    const float cov01 = dot3f(T00, T01, T02, VT01, VT11, VT21);
    const float cov11 = dot3f(T10, T11, T12, VT01, VT11, VT21) + 0.3f;

    // ---- DecomposeCovariance (#else branch)
    const float mid = 0.5f * (cov00 + cov11);
    const float hx = (cov00 - cov11) / 2.0f;
    const float radius = sqrtf(dot2f(hx, cov01, hx, cov01));
    const float lambda1 = mid + radius;
    const float lambda2 = fmaxf(mid - radius, 0.1f);
    float dvx = cov01, dvy = lambda1 - cov00;
    const float invLen = 1.0f / sqrtf(dot2f(dvx, dvy, dvx, dvy));
    dvx *= invLen; dvy *= invLen;
    dvy = -dvy;
    const float s1 = fminf(sqrtf(2.0f * lambda1), 4096.0f), s2 = fminf(sqrtf(2.0f * lambda2), 4096.0f);
    view.axis1[0] = s1 * dvx; view.axis1[1] = s1 * dvy;
    view.axis2[0] = s2 * dvy; view.axis2[1] = s2 * (-dvx);

    // ---- opacity (the colour's alpha half; rgb is added by CalcViewColor)
    const float al = fminf(col.w * P.opacityScale, 65000.0f);
    view.color[1] = f32tof16(al);
}

// SH coefficients are consumed in order sh1..sh15 by three fmaf chains (degree 1, 2, 3), so they are decoded
// one at a time instead of being held in 45 registers.
template <class F = RuntimeFormats, class SHSource>
GS_HD void CalcViewColor(const AssetView& a, const FrameConsts& P, uint32_t idx, ViewPartial& vp, SHSource& shsrc) {
    ViewData& view = vp.view;
    const V4 col = vp.col;
    const V3 shMin = vp.shMin, shMax = vp.shMax;
    const bool shLerp = vp.shLerp;
    const float wx = vp.wx, wy = vp.wy, wz = vp.wz;
    // ---- view direction in object space, SH basis
    const float dwx = P.camx - wx, dwy = P.camy - wy, dwz = P.camz - wz;
    float ox = mrow3(P.w2o, 0, dwx, dwy, dwz), oy = mrow3(P.w2o, 1, dwx, dwy, dwz), oz = mrow3(P.w2o, 2, dwx, dwy, dwz);
    const float invN = 1.0f / sqrtf(dot3f(ox, oy, oz, ox, oy, oz));
    ox *= invN; oy *= invN; oz *= invN;
    const float dx = -ox, dy = -oy, dz = -oz;

    const bool onlySH = P.shOnly != 0;
    // (r, g) travel as a 2-vector (packed fp32 instructions on the device), b alone; every channel sees exactly the
    // operations of ShadeSH in the same order
    F2 rg = onlySH ? F2{ 0.5f, 0.5f } : F2{ col.x, col.y };
    float b = onlySH ? 0.5f : col.z;
    if (P.shOrder >= 1) {
        uint32_t shIndex = idx;
        if (F::shFmt(a) > 3) shIndex = LoadUShort(a.other, vp.otherEnd - 2);
        shsrc.begin(a.sh + (uint64_t)shIndex * shStrideOf(F::shFmt(a)), F::shFmt(a));
        const F2 minRG = { shMin.x, shMin.y }, dRG = F2{ shMax.x, shMax.y } - minRG;      // lerp(a, b, t) = fma(t, b - a, a)
        const float minB = shMin.z, dB = shMax.z - shMin.z;
        auto SHK = [&](int k) -> RGB {
            RGB s = shsrc.load_rgb(k);
            if (shLerp) { s.rg = fma2(s.rg, dRG, minRG); s.b = fmaf(s.b, dB, minB); }
            return s;
        };
        auto MUL = [](float w, const RGB& s) -> RGB { return { F2{ w, w } * s.rg, w * s.b }; };
        auto FMA = [](float w, const RGB& s, const RGB& acc) -> RGB { return { fma2(F2{ w, w }, s.rg, acc.rg), fmaf(w, s.b, acc.b) }; };
        {   // degree 1: res += C1 * (-sh1*y + sh2*z - sh3*x)
            const RGB s1v = SHK(1), s2v = SHK(2), s3v = SHK(3);
            RGB t = MUL(dy, RGB{ -s1v.rg, -s1v.b });
            t = FMA(dz, s2v, t);
            t = FMA(dx, RGB{ -s3v.rg, -s3v.b }, t);
            rg = fma2(F2{ GS_SH_C1, GS_SH_C1 }, t.rg, rg); b = fmaf(GS_SH_C1, t.b, b);
        }
        if (P.shOrder >= 2) {
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const float xy = dx * dy, yz = dy * dz, xz = dx * dz;
            {
                const float b4 = 1.0925484f * xy, b5 = -1.0925484f * yz, b6 = 0.3153916f * (fmaf(2.0f, zz, -xx) - yy),
                            b7 = -1.0925484f * xz, b8 = 0.5462742f * (xx - yy);
                RGB acc = MUL(b4, SHK(4));
                acc = FMA(b5, SHK(5), acc);
                acc = FMA(b6, SHK(6), acc);
                acc = FMA(b7, SHK(7), acc);
                acc = FMA(b8, SHK(8), acc);
                rg += acc.rg; b += acc.b;
            }
            if (P.shOrder >= 3) {
                const float b9 = (-0.5900436f * dy) * fmaf(3.0f, xx, -yy);
                const float b10 = (2.8906114f * xy) * dz;
                const float b11 = (-0.4570458f * dy) * (fmaf(4.0f, zz, -xx) - yy);
                const float b12 = (0.3731763f * dz) * (fmaf(2.0f, zz, -3.0f * xx) - 3.0f * yy);
                const float b13 = (-0.4570458f * dx) * (fmaf(4.0f, zz, -xx) - yy);
                const float b14 = (1.4453057f * dz) * (xx - yy);
                const float b15 = (-0.5900436f * dx) * fmaf(-3.0f, yy, xx);
                RGB acc = MUL(b9, SHK(9));
                acc = FMA(b10, SHK(10), acc);
                acc = FMA(b11, SHK(11), acc);
                acc = FMA(b12, SHK(12), acc);
                acc = FMA(b13, SHK(13), acc);
                acc = FMA(b14, SHK(14), acc);
                acc = FMA(b15, SHK(15), acc);
                rg += acc.rg; b += acc.b;
            }
        }
    }
    float r = rg.x, g = rg.y;
    r = fmaxf(r, 0.0f); g = fmaxf(g, 0.0f); b = fmaxf(b, 0.0f);
    view.color[0] = (f32tof16(r) << 16) | f32tof16(g);
    view.color[1] = (f32tof16(b) << 16) | (view.color[1] & 0xffffu);
}

template <class SHSource>
GS_HD ViewData CalcViewDataT(const AssetView& a, const FrameConsts& P, const EditView& E, uint32_t idx, SHSource& shsrc) {
    ViewPartial vp;
    CalcViewGeom(a, P, E, idx, vp);
    if (vp.front) CalcViewColor(a, P, idx, vp, shsrc);
    return vp.view;
}

GS_HD ViewData CalcViewData(const AssetView& a, const FrameConsts& P, const EditView& E, uint32_t idx) {
    SHFromBlob src;
    return CalcViewDataT(a, P, E, idx, src);
}

// ---- compositor set-up: which splats are drawn, where, and which pixels (hence tiles) they can touch -----------
// Restates the vertex stage of RenderGaussianSplats.shader:35-77 plus the fixed-function clipping it relies
// on (DESIGN.md "compositor semantics"); must stay in step with prepare() in oracle/gs_oracle.cpp.
GS_HD void PixRange(float c, float e, float size, int& lo, int& hi) {
    float flo = ceilf((c - e) - 0.5f), fhi = floorf((c + e) - 0.5f);
    flo = fmaxf(flo, 0.0f); fhi = fminf(fhi, size - 1.0f);
    if (!(flo <= fhi)) { lo = 1; hi = 0; return; }
    lo = (int)flo; hi = (int)fhi;
}

// ---- the fragment's discard decision, made identical on the CPU and the GPU ---------------------------------------
// frag() discards alpha < 1/255 (RenderGaussianSplats.shader:100).  alpha = saturate(exp(power) * a) goes through the one
// operation of the frame that is not bit-identical on both sides (the GPU's exp2 unit vs a correctly rounded exp2, <= 1 ulp),
// so a fragment whose alpha lands within that ulp of 1/255 would be kept on one side and discarded on the other.  Instead,
// when alpha comes out within kAlphaWindow / 2 ulps of 1/255 (about 10^-6 of the fragments) BOTH sides recompute it from
// Exp2Det, an exp2 made of fp32 operations only (the same bits everywhere), and decide on that.  Outside the window the native
// alpha is at least 8 ulps away from the threshold: no 1-ulp difference can change the decision.
constexpr uint32_t kAlphaThresholdBits = 0x3B808081u;                  // 1.0f / 255.0f
constexpr uint32_t kAlphaWindow = 16u;                                 // [1/255 - 8 ulp, 1/255 + 8 ulp)
constexpr uint32_t kAlphaWindowLo = kAlphaThresholdBits - kAlphaWindow / 2u;
// 2^y for y in (-126, 0]: n = rint(y), 2^(y - n) by the degree-7 Taylor polynomial of 2^f on [-0.5, 0.5] (|error| < 1 ulp), exact scaling
GS_HD float Exp2Det(float y) {
    const float n = rintf(y);
    const float f = y - n;
    float p = 1.525273380405984e-05f;
    p = fmaf(p, f, 1.5403530393381608e-04f);
    p = fmaf(p, f, 1.3333558146428443e-03f);
    p = fmaf(p, f, 9.618129107628477e-03f);
    p = fmaf(p, f, 5.550410866482158e-02f);
    p = fmaf(p, f, 2.402265069591007e-01f);
    p = fmaf(p, f, 6.931471805599453e-01f);
    p = fmaf(p, f, 1.0f);
    return ldexpf(p, (int)n);
}
// alpha of a fragment given the native alpha (= saturate(exp2(y) * a) with whatever exp2 the machine has), y = power * log2(e)
// and the splat's opacity a: returns the alpha to blend with, `live` = the fragment is not discarded.
GS_HD float DecideAlpha(float alphaNative, float y, float a, bool& live) {
    const uint32_t u = f2u(alphaNative) - kAlphaWindowLo;
    if (u < kAlphaWindow) {
        const float ad = fminf(fmaxf(Exp2Det(y) * a, 0.0f), 1.0f);
        live = ad >= u2f(kAlphaThresholdBits);
        return ad;
    }
    live = (int32_t)u >= (int32_t)kAlphaWindow;
    return alphaNative;
}

// ---- the fragment of a SELECTED splat (RenderGaussianSplats.shader:87-101) ---------------------------------------------------------
// vert() hands frag() col.a = -1 for a splat whose bit in _SplatSelectedBits is set (:63-73); the splat's own opacity then plays no part.
// With e = exp(-dot(pos, pos)) (half is float here):
//     alpha = e;  if (e > 7/255) { if (e < 10/255) { alpha = 1; rgb = (1, 0, 1); }  alpha = saturate(alpha + 0.3); }
//     rgb = lerp(rgb, (1, 0, 1), 0.5);  discard if alpha < 1/255;  output (rgb alpha, alpha)
// i.e. a magenta tint, raised opacity and a solid magenta ring where e is in (7/255, 10/255).  Literals are fp32 and folded as fp32
// (7.0f / 255.0f ...), lerp is one fmaf, as oracle/_ref's fused build of the shader text evaluates them.
// The three decisions on e are jumps of the OUTPUT (alpha 0.027 -> 1 -> 0.34 across the ring), and e comes from the one operation that is
// not bit-identical on the host and the GPU (exp2, <= 1 ulp apart).  So, as DecideAlpha does for alpha at 1/255: when the native e lies
// within kAlphaWindow / 2 ulps of ANY of the three thresholds, both sides recompute e = Exp2Det(y) and take all three decisions, and the
// alpha, from that.  Outside the windows the native e is >= 8 ulps away from every threshold: no 1-ulp difference changes a decision.
constexpr uint32_t kSelRingLoBits = 0x3CE0E0E1u;                       // 7.0f / 255.0f
constexpr uint32_t kSelRingHiBits = 0x3D20A0A1u;                       // 10.0f / 255.0f
GS_HD bool SplatSelected(const EditView& E, uint32_t idx) { return E.selectedBits && ((E.selectedBits[idx >> 5] >> (idx & 31u)) & 1u); }
// The alpha half of a selected splat's raster record: -1.0 (what vert() puts into col.a).  The blend recognises it by the sign.
constexpr uint32_t kSelectedAlphaHalf = 0xBC00u;
GS_HD bool SelectedNearThreshold(float eNative) {
    const uint32_t b = f2u(eNative), h = kAlphaWindow / 2u;
    return (b - (kAlphaThresholdBits - h) < kAlphaWindow) | (b - (kSelRingLoBits - h) < kAlphaWindow) | (b - (kSelRingHiBits - h) < kAlphaWindow);
}
// eNative = exp2(y) with whatever exp2 the machine has, y = power * log2(e).  Returns the alpha to blend with; ring = the fragment lies on the
// outline ring (its colour is (1, 0, 1) before the tint); live = not discarded.  windowed = false: the shader's arithmetic alone.
GS_HD float DecideSelected(float eNative, float y, bool& ring, bool& live, bool windowed = true) {
    float e = eNative;
    if (windowed && SelectedNearThreshold(eNative)) e = Exp2Det(y);
    float alpha = e;
    ring = false;
    if (e > u2f(kSelRingLoBits)) {
        if (e < u2f(kSelRingHiBits)) { alpha = 1.0f; ring = true; }
        alpha = fminf(fmaxf(alpha + 0.3f, 0.0f), 1.0f);
    }
    live = alpha >= u2f(kAlphaThresholdBits);
    return alpha;
}
// The whole selected fragment: rgb = the splat's colour, out4 = (rgb alpha, alpha) premultiplied in fp32.  Returns live.
GS_HD bool SelectedFragment(float eNative, float y, float r, float g, float b, float* out4, bool windowed = true) {
    bool ring, live;
    const float alpha = DecideSelected(eNative, y, ring, live, windowed);
    if (ring) { r = 1.0f; g = 0.0f; b = 1.0f; }
    r = fmaf(0.5f, 1.0f - r, r); g = fmaf(0.5f, 0.0f - g, g); b = fmaf(0.5f, 1.0f - b, b);      // lerp(rgb, (1, 0, 1), 0.5)
    out4[0] = r * alpha; out4[1] = g * alpha; out4[2] = b * alpha; out4[3] = alpha;
    return live;
}

// ln(x) for a positive normal x from fp32 operations only (bit manipulation, one division, explicit fmaf): the same bits
// on the host and on the device, unlike logf().  |error| < 1e-6 (atanh series of the mantissa reduced to [0.707, 1.414)).
GS_HD float LogDetCore(uint32_t u, int ebias) {                 // u: the bits of a positive normal float; ebias: -127 (or -150 for a denormal scaled by 2^23)
    float e = (float)((int)(u >> 23) + ebias);
    float m = u2f((u & 0x7fffffu) | 0x3f800000u);
    if (m > 1.41421356f) { m *= 0.5f; e += 1.0f; }
    const float t = (m - 1.0f) / (m + 1.0f);
    const float t2 = t * t;
    const float p = fmaf(t2, fmaf(t2, fmaf(t2, 1.0f / 7.0f, 0.2f), 1.0f / 3.0f), 1.0f);
    return fmaf(e, 0.69314718f, (2.0f * t) * p);
}
GS_HD float LogDet(float x) { return LogDetCore(f2u(x), -127); }

// Can the splat put a live fragment on a pixel centre of the square block of pixel centres [bc - half, bc + half]^2 ?
// A fragment is live iff |q1| <= 2, |q2| <= 2 and exp(-(q1^2+q2^2)) a >= 1/255, q_k = u_k . (p - c)  (frag, :79-106).
// q_k is linear in p, so min |q_k| over the block is closed form (separating-axis test along u_1 and u_2); the block is
// rejected when even those minima violate one of the three conditions.  Conservative: never rejects a live fragment
// (r2 carries the slack for the fp32 rounding of this test and of the kernel's exp).
GS_HD bool BlockMayTouch(float bcx, float bcy, float half, float cx, float cy, float u1x, float u1y, float u2x, float u2y, float r2) {
    const float dx = bcx - cx, dy = bcy - cy;
    const float d1 = fabsf(fmaf(dy, u1y, dx * u1x)) - half * (fabsf(u1x) + fabsf(u1y));
    const float d2 = fabsf(fmaf(dy, u2y, dx * u2x)) - half * (fabsf(u2x) + fabsf(u2y));
    const float m1 = fmaxf(d1, 0.0f), m2 = fmaxf(d2, 0.0f);
    return (m1 <= 2.001f) && (m2 <= 2.001f) && (fmaf(m2, m2, m1 * m1) <= r2);
}

struct SplatFootprint {
    float cx, cy;               // centre in pixels, y down
    int x0, x1, y0, y1;         // inclusive PIXEL rect of the tight footprint, clamped to the screen (x0 > x1: nothing to draw); the
                                // compositor's tile rectangle is this shifted by the tile shape the draw picks (x >> log2 tile width ...)
};
// The 8-byte per-splat rectangle calc_view leaves for the binning: x = x0 | y0 << 16, y = (x1 + 1) | (y1 + 1) << 16 (pixels; targets are
// at most 65535 pixels wide / high); all zero = not drawn.
GS_HD void PackPixelRect(const SplatFootprint& fp, uint32_t& rx, uint32_t& ry) {
    rx = (uint32_t)fp.x0 | ((uint32_t)fp.y0 << 16);
    ry = (uint32_t)(fp.x1 + 1) | ((uint32_t)(fp.y1 + 1) << 16);
}

GS_HD bool PrepareSplat(const ViewData& v, float W, float H, float nearClip, float farClip, SplatFootprint& fp) {
    fp.x0 = 1; fp.x1 = 0; fp.y0 = 1; fp.y1 = 0; fp.cx = 0.0f; fp.cy = 0.0f;
    const float w = v.pos[3];
    const float a = f16tof32(v.color[1]);
    // the rejections are evaluated as ONE predicate (bitwise &: no short-circuit): a chain of early returns compiles to
    // nested divergent branches that each re-materialise the "culled" outputs
    const int drawable = (int)(w > 0.0f) & (int)(w >= nearClip) & (int)(w <= farClip) & (int)finite32(v.axis1[0]) & (int)finite32(v.axis1[1]) &
                         (int)finite32(v.axis2[0]) & (int)finite32(v.axis2[1]) & (int)(a >= 1.0f / 255.0f);
    if (!drawable) return false;
    const float invw = 1.0f / w;
    const float cx = fmaf(0.5f * (v.pos[0] * invw), W, 0.5f * W);
    const float cy = fmaf(-0.5f * (v.pos[1] * invw), H, 0.5f * H);
    const float a1x = v.axis1[0], a1y = v.axis1[1], a2x = v.axis2[0], a2y = v.axis2[1];
    // the oracle's prepare() rejects a splat whose 1 / |axis_k|^2 is not finite (the blend divides by it).  |axis|^2 = d is a sum of two
    // squares (never negative), and fl(1 / d) is finite exactly when d is +inf or 2^-128 < d < inf and not NaN (1 / 2^-128 = 2^128
    // overflows, the next denormal up does not): an integer range test on the bits instead of two IEEE divisions (~22 VALU each)
    const float d1 = dot2f(a1x, a1y, a1x, a1y), d2 = dot2f(a2x, a2y, a2x, a2y);
    const int inv1ok = (int)((f2u(d1) - 0x00200001u) <= (0x7f800000u - 0x00200001u)), inv2ok = (int)((f2u(d2) - 0x00200001u) <= (0x7f800000u - 0x00200001u));
    fp.cx = cx; fp.cy = cy;                                         // (only read when the splat turns out visible)
    if (!((int)finite32(cx) & (int)finite32(cy) & inv1ok & inv2ok)) return false;
    const float exr = 2.0f * (fabsf(a1x) + fabsf(a2x)), eyr = 2.0f * (fabsf(a1y) + fabsf(a2y));
    const float slack = 0.01f;
    int x0, x1, y0, y1;
    PixRange(fp.cx, exr + slack, W, x0, x1);
    PixRange(fp.cy, eyr + slack, H, y0, y1);
    if (x0 > x1 || y0 > y1) return false;
    const float r2 = fmaf(LogDet(255.0f * a), 1.0001f, 1.0e-3f);
    const float rr = sqrtf(fmaxf(r2, 0.0f));
    const float exe = rr * sqrtf(dot2f(a1x, a2x, a1x, a2x)), eye = rr * sqrtf(dot2f(a1y, a2y, a1y, a2y));
    PixRange(fp.cx, fminf(exr, exe) + slack, W, x0, x1);
    PixRange(fp.cy, fminf(eyr, eye) + slack, H, y0, y1);
    if (x0 > x1 || y0 > y1) return true;         // drawn by the reference, but every fragment is below 1/255
    fp.x0 = x0; fp.x1 = x1; fp.y0 = y0; fp.y1 = y1;
    return true;
}

// PrepareSplat for a draw that highlights the selection.  A SELECTED splat's visibility and pixel rectangle are those of opacity 1 -- no
// opacity cull, r2 from a = 1 -- because its fragments are live wherever e >= 1/255 inside the quad, whatever the splat's own opacity
// (DecideSelected).  The view record itself is not changed; an unselected splat is PrepareSplat's, bit for bit.
GS_HD bool PrepareSplatHighlight(const ViewData& v, bool selected, float W, float H, float nearClip, float farClip, SplatFootprint& fp) {
    ViewData o = v;
    if (selected) o.color[1] = (v.color[1] & 0xffff0000u) | 0x3C00u;
    return PrepareSplat(o, W, H, nearClip, farClip, fp);
}
// ... and the colour dword of its raster record: the alpha half becomes vert()'s col.a = -1
GS_HD uint32_t RecordColor1(uint32_t color1, bool selected) { return selected ? ((color1 & 0xffff0000u) | kSelectedAlphaHalf) : color1; }

// ---- export: CSExportData (SplatUtilities.compute:523-673; kernels in gs_export.hip) ---------------------------------------------
// LogDet over every float: the IEEE results for the special inputs (-inf for +-0, NaN for a negative or NaN input, +inf for +inf), a
// denormal input scaled by 2^23 first (exact), LogDet's construction otherwise -- so a positive normal x gives LogDet(x)'s bits.  HLSL's
// log is a family of results (an approximation per vendor); this is the member the project fixes: fp32 operations only, one rounding each,
// so the GPU, the host build and the numpy twin (creator.LogDet, which states and derives the error bound) agree bit for bit.
GS_HD float LogDetFull(float x) {
    const uint32_t u = f2u(x);
    if (u >= 0x7f800000u) {                                        // +inf, NaN, or the sign bit set
        if ((u << 1) == 0u) return u2f(0xff800000u);               // -0
        if (u == 0x7f800000u) return x;
        return u2f(0x7fc00000u);
    }
    if (u == 0u) return u2f(0xff800000u);
    if (u < 0x00800000u) return LogDetCore(f2u(x * 8388608.0f), -150);
    return LogDetCore(u, -127);
}

// LoadSplatData (GaussianSplatting.hlsl:428-608), every field: the one consumer of the full decode is the export
struct SplatFull { V3 pos; V4 rot; V3 scale; float opacity; V3 col; V3 sh[15]; };
GS_HD void LoadSplatDataFull(const AssetView& a, uint32_t idx, uint32_t ci, const V3& pos, SplatFull& s) {
    s.pos = pos;                                                   // LoadSplatPosChunk(a, idx, ci), loaded by the caller for its cut test
    uint32_t otherStride = 4 + vecStride(a.scaleFmt);
    if (a.shFmt > 3) otherStride += 2;
    const uint64_t otherAddr = (uint64_t)idx * otherStride;
    s.rot = DecodeRotation(LoadUInt(a.other, otherAddr));
    s.scale = LoadVec(a.other, otherAddr + 4, a.scaleFmt);
    V4 col = LoadColorTexel(a, idx);
    uint32_t shIndex = idx;
    if (a.shFmt > 3) shIndex = LoadUShort(a.other, otherAddr + otherStride - 2);      // Cluster*: the palette index first, the gather second
    const uint8_t* sp = a.sh + (uint64_t)shIndex * shStrideOf(a.shFmt);
#pragma unroll
    for (int k = 0; k < 15; ++k) s.sh[k] = LoadSH(sp, a.shFmt, k + 1);
    if (ci < a.chunkCount) {
        const ChunkRaw ck = LoadChunk(a.chunk, ci);
        s.scale.x = lerpf(f16tof32(ck.w[10]), f16tof32(ck.w[10] >> 16), s.scale.x);
        s.scale.y = lerpf(f16tof32(ck.w[11]), f16tof32(ck.w[11] >> 16), s.scale.y);
        s.scale.z = lerpf(f16tof32(ck.w[12]), f16tof32(ck.w[12] >> 16), s.scale.z);
        s.scale.x *= s.scale.x; s.scale.y *= s.scale.y; s.scale.z *= s.scale.z;
        s.scale.x *= s.scale.x; s.scale.y *= s.scale.y; s.scale.z *= s.scale.z;
        s.scale.x *= s.scale.x; s.scale.y *= s.scale.y; s.scale.z *= s.scale.z;
        col.x = lerpf(f16tof32(ck.w[0]), f16tof32(ck.w[0] >> 16), col.x);
        col.y = lerpf(f16tof32(ck.w[1]), f16tof32(ck.w[1] >> 16), col.y);
        col.z = lerpf(f16tof32(ck.w[2]), f16tof32(ck.w[2] >> 16), col.z);
        col.w = lerpf(f16tof32(ck.w[3]), f16tof32(ck.w[3] >> 16), col.w);
        col.w = InvSquareCentered01(col.w);
        if (a.shFmt > 0 && a.shFmt <= 3) {
            const V3 lo = { f16tof32(ck.w[13]), f16tof32(ck.w[14]), f16tof32(ck.w[15]) };
            const V3 hi = { f16tof32(ck.w[13] >> 16), f16tof32(ck.w[14] >> 16), f16tof32(ck.w[15] >> 16) };
#pragma unroll
            for (int k = 0; k < 15; ++k) s.sh[k] = { lerpf(lo.x, hi.x, s.sh[k].x), lerpf(lo.y, hi.y, s.sh[k].y), lerpf(lo.z, hi.z, s.sh[k].z) };
        }
    }
    s.opacity = col.w;
    s.col = { col.x, col.y, col.z };
}

// The band matrices of RotateSH (SphericalHarmonics.hlsl:24-210) for the matrix of CalcSHRotMatrix (SplatUtilities.compute:588-609).  The
// reference rebuilds them in every thread; they depend on the dispatch's matrix only, so the host builds them once per call with this
// function and the kernel receives the 83 floats by value.
// Formulation (the project's own; the reference unrolls the same recurrence into 74 closed expressions): the Ivanic-Ruedenberg recurrence
// for real spherical harmonics (J. Phys. Chem. 100 (1996) 6342, with the 1998 errata).  With R the band-1 matrix (rows / columns m, n = -1, 0, 1)
// and M the matrix of band l - 1, entry (m, n) of band l, m, n = -l .. l, is a sum of at most five terms c * P_i(a, n):
//     P_i(a, n) = R(i, 0) M(a, n)                                  for |n| < l
//               = R(i, 1) M(a, l - 1) - R(i, -1) M(a, -l + 1)      for n = l
//               = R(i, 1) M(a, -l + 1) + R(i, -1) M(a, l - 1)      for n = -l
//     d = (l + n)(l - n) for |n| < l, else 2l (2l - 1);  u = sqrt((l + m)(l - m) / d);  v = sqrt((l + |m| - 1)(l + |m|) / d) / 2;
//     w = -sqrt((l - |m| - 1)(l - |m|) / d) / 2
//     m = 0:  u P_0(0), -v sqrt2 P_1(1), -v sqrt2 P_-1(-1)
//     m > 0:  u P_0(m), v sqrt(1 + [m = 1]) P_1(m - 1), -v [m != 1] P_-1(-m + 1), w P_1(m + 1), w P_-1(-m - 1)
//     m < 0:  u P_0(m), v [m != -1] P_1(m + 1), v sqrt(1 + [m = -1]) P_-1(-m - 1), w P_1(m - 1), -w P_-1(-m + 1)
// Operation order (what makes the bits a function of this text): every coefficient c is formed in fp64 -- the ratio, its square root, the
// factor 1/2, the factor sqrt2 where it applies, the sign -- and rounded to fp32 once; a term whose fp32 coefficient is zero is skipped;
// P_i is one fp32 product, or two products and their sum / difference; the terms are c * P, added left to right in the order listed.
// The band-1 matrix carries the signs of ShadeSH's basis (-y, z, -x), as the reference's does (SphericalHarmonics.hlsl:76-83); length() is
// sqrt((x x + y y) + z z).  Choices of one member of a family, as with LogDet.
struct SHRot { float sh1[3][3]; float sh2[5][5]; float sh3[7][7]; };
GS_HD float SHRotP(const float (*r1)[3], const float* prev, int l, int i, int a, int n) {
    const int w = 2 * l - 1, c = l - 1;                             // prev: (2l - 1) x (2l - 1), index = value + l - 1
    const float* row = prev + (a + c) * w;
    if (n == l) return r1[i + 1][2] * row[2 * c] - r1[i + 1][0] * row[0];
    if (n == -l) return r1[i + 1][2] * row[0] + r1[i + 1][0] * row[2 * c];
    return r1[i + 1][1] * row[n + c];
}
struct SHRotSum {                                                  // the running sum of one entry
    const float (*r1)[3]; const float* prev; int l, n; float acc; bool any;
    GS_HD void add(double c64, int i, int a) {
        const float c = (float)c64;
        if (c == 0.0f) return;                                     // (also what keeps P_i(a, n) inside band l - 1: |a| = l only ever meets c = 0)
        const float t = c * SHRotP(r1, prev, l, i, a, n);
        acc = any ? acc + t : t;
        any = true;
    }
};
GS_HD void SHRotBand(const float (*r1)[3], const float* prev, int l, float* out) {
    const double sqrt2 = sqrt(2.0);
    for (int m = -l; m <= l; ++m)
        for (int n = -l; n <= l; ++n) {
            const int am = m < 0 ? -m : m, an = n < 0 ? -n : n;
            const double d = an < l ? (double)((l + n) * (l - n)) : (double)(2 * l * (2 * l - 1));
            const double u = sqrt((double)((l + m) * (l - m)) / d);
            const double v = sqrt((double)((l + am - 1) * (l + am)) / d) * 0.5;
            const double w = -(sqrt((double)((l - am - 1) * (l - am)) / d) * 0.5);
            SHRotSum s = { r1, prev, l, n, 0.0f, false };
            s.add(u, 0, m);
            if (m == 0) { s.add(-(v * sqrt2), 1, 1); s.add(-(v * sqrt2), -1, -1); }
            else if (m > 0) { s.add(m == 1 ? v * sqrt2 : v, 1, m - 1); if (m != 1) s.add(-v, -1, -m + 1); s.add(w, 1, m + 1); s.add(w, -1, -m - 1); }
            else { if (m != -1) s.add(v, 1, m + 1); s.add(m == -1 ? v * sqrt2 : v, -1, -m - 1); s.add(w, 1, m - 1); s.add(-w, -1, -m + 1); }
            out[(m + l) * (2 * l + 1) + (n + l)] = s.any ? s.acc : 0.0f;
        }
}
// CalcSHRotMatrix (SplatUtilities.compute:588-609): the rows of the 3x3 part, each divided by its length
GS_HD void SHRotMatrix(const float* o2w, float (*m)[3]) {          // o2w: _MatrixObjectToWorld, rows of 4
    for (int r = 0; r < 3; ++r) {
        const float x = o2w[r * 4], y = o2w[r * 4 + 1], z = o2w[r * 4 + 2];
        const float inv = 1.0f / sqrtf((x * x + y * y) + z * z);
        m[r][0] = x * inv; m[r][1] = y * inv; m[r][2] = z * inv;
    }
}
GS_HD void CalcSHRot(const float* o2w, SHRot& R) {
    float m[3][3];
    SHRotMatrix(o2w, m);
    // band 1: rows / columns in the order y, z, x of the real harmonics, with the basis' signs
    R.sh1[0][0] = m[1][1]; R.sh1[0][1] = -m[1][2]; R.sh1[0][2] = m[1][0];
    R.sh1[1][0] = -m[2][1]; R.sh1[1][1] = m[2][2]; R.sh1[1][2] = -m[2][0];
    R.sh1[2][0] = m[0][1]; R.sh1[2][1] = -m[0][2]; R.sh1[2][2] = m[0][0];
    SHRotBand(R.sh1, &R.sh1[0][0], 2, &R.sh2[0][0]);
    SHRotBand(R.sh1, &R.sh2[0][0], 3, &R.sh3[0][0]);
}

// what CSExportData reads of its dispatch: _ExportTransformFlags, _MatrixObjectToWorld (rows 0..2), _ExportTransformRotation (xyzw),
// _ExportTransformScale, and the band matrices of the matrix
struct ExportXform { uint32_t bake; float o2w[12]; float rot[4]; float scale[3]; SHRot sh; };

// Dot3 / Dot5 / Dot7 of RotateSH (SphericalHarmonics.hlsl:11-22) for one output coefficient: products and sums one by one, left to right
GS_HD V3 SHDotRow(const V3* v, const float* f, int n) {
    V3 r = { v[0].x * f[0], v[0].y * f[0], v[0].z * f[0] };
    for (int k = 1; k < n; ++k) { r.x = r.x + v[k].x * f[k]; r.y = r.y + v[k].y * f[k]; r.z = r.z + v[k].z * f[k]; }
    return r;
}

// The transform CSExportData bakes (SplatUtilities.compute:627-643) and CSCopySplats applies (:699-712), the same text in both: position through the
// matrix (m: rows 0..2), the axis flips of a negative scale, QuatMul(rot, .), scale *= |scale|, RotateSH with the band matrices of the matrix.
// The three pieces after the flips stand on their own: the rigid rotate / scale of the selection (EditRigid*, above the kernels of gs_edit.hip)
// applies them to the mouse-down state of a selected splat, so that an edited splat and a merged one are the same arithmetic.
GS_HD V4 BakeQuat(const float* rot, const V4& q) { return QuatMul({ rot[0], rot[1], rot[2], rot[3] }, q); }
GS_HD V3 BakeScale(const V3& s, const float* scale) { return { s.x * fabsf(scale[0]), s.y * fabsf(scale[1]), s.z * fabsf(scale[2]) }; }
// one band of RotateSH (SphericalHarmonics.hlsl:24-210): N = 3, 5, 7 coefficients in, as many out
template <int N> GS_HD void RotateSHBand(const V3* in, const float (*f)[N], V3* out) {
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = SHDotRow(in, f[k], N);
}
GS_HD void BakeSplatTransform(SplatFull& s, const float* m, const float* rot, const float* scale, const SHRot& sh) {
    const V3 pos = s.pos;
    s.pos = { mrow(m, 0, pos.x, pos.y, pos.z), mrow(m, 1, pos.x, pos.y, pos.z), mrow(m, 2, pos.x, pos.y, pos.z) };
    // (this only handles axis flips from scale, not any arbitrary scaling: the reference's note)
    if (scale[0] < 0.0f) { s.rot.y = -s.rot.y; s.rot.z = -s.rot.z; }
    if (scale[1] < 0.0f) { s.rot.x = -s.rot.x; s.rot.z = -s.rot.z; }
    if (scale[2] < 0.0f) { s.rot.x = -s.rot.x; s.rot.y = -s.rot.y; }
    s.rot = BakeQuat(rot, s.rot);
    s.scale = BakeScale(s.scale, scale);
    V3 out[15];
    RotateSHBand<3>(s.sh, sh.sh1, out);
    RotateSHBand<5>(s.sh + 3, sh.sh2, out + 3);
    RotateSHBand<7>(s.sh + 8, sh.sh3, out + 8);
#pragma unroll
    for (int k = 0; k < 15; ++k) s.sh[k] = out[k];
}

// ---- rigid rotate / scale of the selection (gs_renderer_edit_set_rigid_transforms; kernels in gs_edit.hip) --------
// What the reference's three @TODOs leave out, for one selected splat, from its mouse-down state.  q: the quaternion of the linear part L of the
// position map, sh: the band matrices of L, both made once per call on the host (gs::edit_rigid_of, gs_params.h); s: the uniform scale factor.
struct EditRigid { float q[4]; float s; SHRot sh; };
// the rotation word: QuatMul(q_L, rot) -- the side BakeSplatTransform multiplies on, not CSRotateSelection's
GS_HD uint32_t EditRigidRotateWord(const EditRigid& G, uint32_t mouseDown) {
    return EncodeQuatToNorm10(PackSmallest3Rotation(BakeQuat(G.q, DecodeRotation(mouseDown))));
}
// the three fp32 scales: each times |s|, one product
GS_HD V3 EditRigidScale(const EditRigid& G, const V3& mouseDown) {
    const float s3[3] = { G.s, G.s, G.s };
    return BakeScale(mouseDown, s3);
}
// one band of an fp32 SH record (floats, 3 per coefficient; first = 0, 3, 8), read from the mouse-down record and written to the current one
template <int N> GS_HD void EditRigidSHBand(const float* src, float* dst, const float (*f)[N], int first) {
    V3 in[N], out[N];
#pragma unroll
    for (int k = 0; k < N; ++k) in[k] = { src[3 * (first + k)], src[3 * (first + k) + 1], src[3 * (first + k) + 2] };
    RotateSHBand<N>(in, f, out);
#pragma unroll
    for (int k = 0; k < N; ++k) { dst[3 * (first + k)] = out[k].x; dst[3 * (first + k) + 1] = out[k].y; dst[3 * (first + k) + 2] = out[k].z; }
}
// the 45 coefficients of a record: 180 of its 192 bytes; the last 12 are not touched (the copy kernel's rule)
GS_HD void EditRigidRotateSH(const EditRigid& G, const float* src, float* dst) {
    EditRigidSHBand<3>(src, dst, G.sh.sh1, 0);
    EditRigidSHBand<5>(src, dst, G.sh.sh2, 3);
    EditRigidSHBand<7>(src, dst, G.sh.sh3, 8);
}

// The body of CSExportData (SplatUtilities.compute:616-673) for one splat: rec = the 62 floats of ExportSplatData = InputSplatData
// (pos, nor, dc0, 15 R + 15 G + 15 B SH coefficients, opacity, scale, rot wxyz).  pos = LoadSplatPosChunk(a, idx, ci) and cut = IsSplatCut(pos)
// come from the caller, which needs them before it decides whether the splat is exported at all.
// ExportSplatLinear also hands out the decoded linear opacity, the value the logit of rec[54] is taken of (the SPZ writer's alpha: no log between
// the asset and its byte).
GS_HD void ExportSplatLinear(const AssetView& a, const ExportXform& X, uint32_t idx, uint32_t ci, const V3& pos, bool cut, float* rec, float& opacity) {
    SplatFull s;
    LoadSplatDataFull(a, idx, ci, pos, s);
    if (X.bake != 0u) BakeSplatTransform(s, X.o2w, X.rot, X.scale, X.sh);
    const float nor = cut ? 1.0f : 0.0f;                           // mark as skipped for export
    rec[0] = s.pos.x; rec[1] = s.pos.y; rec[2] = s.pos.z;
    rec[3] = nor; rec[4] = nor; rec[5] = nor;
    rec[6] = (s.col.x - 0.5f) / 0.2820948f; rec[7] = (s.col.y - 0.5f) / 0.2820948f; rec[8] = (s.col.z - 0.5f) / 0.2820948f;      // ColorToSH0
#pragma unroll
    for (int k = 0; k < 15; ++k) { rec[9 + k] = s.sh[k].x; rec[24 + k] = s.sh[k].y; rec[39 + k] = s.sh[k].z; }
    rec[54] = LogDetFull(s.opacity / fmaxf(1.0f - s.opacity, 1.0e-6f));                 // InvSigmoid
    rec[55] = LogDetFull(s.scale.x); rec[56] = LogDetFull(s.scale.y); rec[57] = LogDetFull(s.scale.z);
    rec[58] = s.rot.w; rec[59] = s.rot.x; rec[60] = s.rot.y; rec[61] = s.rot.z;
    opacity = s.opacity;
}
GS_HD void ExportSplat(const AssetView& a, const ExportXform& X, uint32_t idx, uint32_t ci, const V3& pos, bool cut, float* rec) {
    float opacity;
    ExportSplatLinear(a, X, idx, ci, pos, cut, rec, opacity);
}

// ---- export to SPZ: the inverse of SpzRecord / spz_read_stream (below; SPZFileReader.cs:26-198), column by column (kernels in gs_export.hip) ----
// Every byte is a function of this text: fp32 operations, each product and each sum rounded on its own, rintf (ties to even) to an integer, and
// no NaN ever converted.  The SH codes are plain roundings: the bucket snapping of the format's original packer is not restated.
constexpr uint32_t kSpzMagic = 0x5053474eu;                        // "NGSP"
constexpr uint32_t kSpzMaxSplats = 10000000u;                      // the readers' limit (SPZFileReader.cs:72)
constexpr uint32_t kSpzFractAuto = 0xffffffffu;
constexpr uint32_t kSpzColumns = 6u;
GS_HD uint32_t SpzShCoeffs(uint32_t level) { return level == 1u ? 3u : (level == 2u ? 8u : (level == 3u ? 15u : 0u)); }
// bytes per splat of column c: positions, alpha, colour, scale, rotation, SH
GS_HD uint32_t SpzColumnWidth(uint32_t c, uint32_t shCoeffs) { return c == 0u ? 9u : (c == 1u ? 1u : (c == 5u ? 3u * shCoeffs : 3u)); }
GS_HD uint32_t SpzCode8(float t) {
    if (!(t >= 0.0f)) return 0u;                                   // NaN, -inf, every negative
    if (t > 255.0f) return 255u;
    return (uint32_t)rintf(t);
}
// one coordinate as 24-bit two's complement fixed point with fractBits (0..24) fractional bits
GS_HD uint32_t SpzPackCoordinate(float p, uint32_t fractBits) {
    const float q = rintf(p * (float)(1u << fractBits));          // the scaling by a power of two is exact
    if (!(q == q)) return 0u;
    if (q < -8388608.0f) return 0x800000u;
    if (q > 8388607.0f) return 0x7fffffu;
    return (uint32_t)(int32_t)q & 0xffffffu;
}
// the automatic fractBits for bounds = min xyz / max xyz of the exported positions: the largest f <= 12 at which the largest |coordinate| still fits
GS_HD uint32_t SpzAutoFractBits(const float* bounds) {
    float m = 0.0f;
    for (int k = 0; k < 6; ++k) m = fmaxf(m, fabsf(bounds[k]));
    for (uint32_t f = 12u; f > 0u; --f)
        if (rintf(m * (float)(1u << f)) <= 8388607.0f) return f;
    return 0u;
}
GS_HD void SpzPackPosition(const float* rec, uint32_t fractBits, uint8_t* out9) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t q = SpzPackCoordinate(rec[c], fractBits);
        out9[c * 3] = (uint8_t)q; out9[c * 3 + 1] = (uint8_t)(q >> 8); out9[c * 3 + 2] = (uint8_t)(q >> 16);
    }
}
GS_HD uint8_t SpzPackAlpha(float linearOpacity) { return (uint8_t)SpzCode8(linearOpacity * 255.0f); }
GS_HD uint8_t SpzPackColor(float dc0) { return (uint8_t)SpzCode8(((dc0 * 0.15f) + 0.5f) * 255.0f); }
GS_HD uint8_t SpzPackScale(float logScale) { return (uint8_t)SpzCode8((logScale + 10.0f) * 16.0f); }
GS_HD uint8_t SpzPackSH(float c) { return (uint8_t)SpzCode8((c * 128.0f) + 128.0f); }
// w, x, y, z of the record -> the x, y, z bytes of the unit quaternion with w >= 0
GS_HD void SpzPackRotation(float w, float x, float y, float z, uint8_t* out3) {
    const float l2 = ((x * x + y * y) + z * z) + w * w;
    const float inv = 1.0f / sqrtf(l2);
    float c[3] = { x * inv, y * inv, z * inv };
    if (w < 0.0f) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) out3[k] = (uint8_t)SpzCode8((c[k] * 127.5f) + 127.5f);
}
// One splat into its place in each of the six columns: rec = the 62 floats of ExportSplatLinear, linearOpacity its second output.  The SH column takes
// the first shCoeffs coefficients as [coefficient][r, g, b]; the record holds them channel-major
GS_HD void SpzPackSplat(const float* rec, float linearOpacity, uint32_t fractBits, uint32_t shCoeffs, uint8_t* pos9, uint8_t* alpha1, uint8_t* col3,
                        uint8_t* scale3, uint8_t* rot3, uint8_t* sh) {
    SpzPackPosition(rec, fractBits, pos9);
    alpha1[0] = SpzPackAlpha(linearOpacity);
#pragma unroll
    for (int c = 0; c < 3; ++c) { col3[c] = SpzPackColor(rec[6 + c]); scale3[c] = SpzPackScale(rec[55 + c]); }
    SpzPackRotation(rec[58], rec[59], rec[60], rec[61], rot3);
#pragma unroll
    for (uint32_t j = 0; j < 15u; ++j) {
        if (j < shCoeffs) {
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) sh[j * 3u + c] = SpzPackSH(rec[9u + c * 15u + j]);
        }
    }
}
// the 16 bytes in front of the columns
GS_HD void SpzHeaderWords(uint32_t n, uint32_t shLevel, uint32_t fractBits, uint32_t* w) { w[0] = kSpzMagic; w[1] = 2u; w[2] = n; w[3] = shLevel | (fractBits << 8); }

// ---- merge: CSCopySplats (SplatUtilities.compute:675-758; kernel in gs_copy.hip) ----------------------------------------------------
// what the kernel reads of its dispatch: _CopyTransformMatrix (rows 0..2), _CopyTransformRotation (xyzw), _CopyTransformScale, and the band
// matrices of the matrix (gsm::CalcSHRot, built once per call on the host)
struct CopyXform { float m[12]; float rot[4]; float scale[3]; SHRot sh; };
// one destination record in the reference's fixed layout (:714-747): pos 12 B; other 16 B = { rotation word, scale.xyz }; the colour texel
// (col.rgb, opacity); 15 x 3 fp32 SH coefficients (the 12 bytes that round an SH record up to 192 are not written)
struct CopyRec { V3 pos; uint32_t rot; V3 scale; V4 color; V3 sh[15]; };
// The body of CSCopySplats for the splat the kernel LOADS: LoadSplatData(idx) (:697) -- the thread index, not srcIdx; the two callers of the
// reference pass _CopySrcStartIndex = 0, where they agree -- transformed like a baked export and re-encoded.  No IsSplatCut: cut splats are copied.
GS_HD void CopySplat(const AssetView& a, const CopyXform& X, uint32_t idx, uint32_t ci, CopyRec& o) {
    SplatFull s;
    LoadSplatDataFull(a, idx, ci, LoadSplatPosChunk(a, idx, ci), s);
    BakeSplatTransform(s, X.m, X.rot, X.scale, X.sh);
    o.pos = s.pos;
    o.rot = EncodeQuatToNorm10(PackSmallest3Rotation(s.rot));
    o.scale = s.scale;
    o.color = { s.col.x, s.col.y, s.col.z, s.opacity };
#pragma unroll
    for (int k = 0; k < 15; ++k) o.sh[k] = s.sh[k];
}

// ---- bake: the per-chunk part of the importer (CalcChunkDataJob and the encoders, GaussianSplatAssetCreator.cs:520-638, 727-758, 776-805,
// 873-932, 934-1037, in the operation order of gs_import.cpp with linearize = 0; kernels in gs_bake.hip) ---------------------------------
// Only + - x /, sqrt, fmin / fmax, fp16 rounding and truncating conversions: a build with -ffp-contract=off gives the host importer's bytes.
// One ambiguity is inherited from fmin / fmax: among values that compare equal they do not pin the sign of zero, so a column that holds both
// +0 and -0 as an extreme may differ in the sign bit of its chunk bound.
constexpr int kBakeCols = 13;                                      // pos 3, scale 3, colour 4 (rgb + opacity), sh 3 (over all 15 coefficients)
struct BakeRec { V3 pos; uint32_t rot; V3 scale; V4 col; float sh[45]; };   // sh: coefficient-major, rgb inside
struct BakeBounds { float mn[kBakeCols], mx[kBakeCols]; };
struct BakeFormats { uint32_t pos, scale, color, sh, chunked; };

// the linear record of one decoded splat.  The rotation word equals the importer's q(rot[k], 1023.5) | ... of PackSmallest3Rotation's output for
// every value inside the field ranges
GS_HD void BakeLinearRecord(const SplatFull& s, BakeRec& o) {
    o.pos = s.pos;
    o.rot = EncodeQuatToNorm10(PackSmallest3Rotation(s.rot));
    o.scale = s.scale;
    o.col = { s.col.x, s.col.y, s.col.z, s.opacity };
#pragma unroll
    for (int k = 0; k < 15; ++k) { o.sh[3 * k] = s.sh[k].x; o.sh[3 * k + 1] = s.sh[k].y; o.sh[3 * k + 2] = s.sh[k].z; }
}
GS_HD float SquareCentered01(float x) { x -= 0.5f; x = x * (x * sgn(x)); return x * 2.0f + 0.5f; }      // GaussianUtils.cs:25-30
// what a chunked asset stores: scale^(1/8) as three square roots, the opacity squared about its centre (:546-548)
GS_HD void BakeChunkSpace(BakeRec& o) {
    o.scale.x = sqrtf(sqrtf(sqrtf(o.scale.x))); o.scale.y = sqrtf(sqrtf(sqrtf(o.scale.y))); o.scale.z = sqrtf(sqrtf(sqrtf(o.scale.z)));
    o.col.w = SquareCentered01(o.col.w);
}
GS_HD void BakeBoundsEmpty(BakeBounds& b) {
    const float inf = u2f(0x7f800000u);
#pragma unroll
    for (int c = 0; c < kBakeCols; ++c) { b.mn[c] = inf; b.mx[c] = -inf; }
}
GS_HD void BakeBoundsMerge(BakeBounds& b, const BakeBounds& o) {
#pragma unroll
    for (int c = 0; c < kBakeCols; ++c) { b.mn[c] = fminf(b.mn[c], o.mn[c]); b.mx[c] = fmaxf(b.mx[c], o.mx[c]); }
}
GS_HD void BakeBoundsOf(const BakeRec& o, BakeBounds& b) {         // the bounds of one splat (in chunk space)
    b.mn[0] = b.mx[0] = o.pos.x; b.mn[1] = b.mx[1] = o.pos.y; b.mn[2] = b.mx[2] = o.pos.z;
    b.mn[3] = b.mx[3] = o.scale.x; b.mn[4] = b.mx[4] = o.scale.y; b.mn[5] = b.mx[5] = o.scale.z;
    b.mn[6] = b.mx[6] = o.col.x; b.mn[7] = b.mx[7] = o.col.y; b.mn[8] = b.mx[8] = o.col.z; b.mn[9] = b.mx[9] = o.col.w;
    const float inf = u2f(0x7f800000u);
    b.mn[10] = b.mn[11] = b.mn[12] = inf; b.mx[10] = b.mx[11] = b.mx[12] = -inf;
#pragma unroll
    for (int k = 0; k < 15; ++k) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { b.mn[10 + d] = fminf(b.mn[10 + d], o.sh[3 * k + d]); b.mx[10 + d] = fmaxf(b.mx[10 + d], o.sh[3 * k + d]); }
    }
}
// make sure the ranges are not empty (:591-594), then the 16-dword ChunkInfo: fp16 pairs for colour, scale and sh, raw fp32 for pos
GS_HD void BakeBoundsWiden(BakeBounds& b) {
#pragma unroll
    for (int c = 0; c < kBakeCols; ++c) b.mx[c] = fmaxf(b.mx[c], b.mn[c] + 1.0e-5f);
}
GS_HD uint32_t BakeHalfPair(float lo, float hi) { return f32tof16(lo) | (f32tof16(hi) << 16); }
GS_HD void BakeChunkWords(const BakeBounds& b, uint32_t* w) {
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = BakeHalfPair(b.mn[6 + d], b.mx[6 + d]);
#pragma unroll
    for (int d = 0; d < 3; ++d) { w[4 + 2 * d] = f2u(b.mn[d]); w[5 + 2 * d] = f2u(b.mx[d]); }
#pragma unroll
    for (int d = 0; d < 3; ++d) w[10 + d] = BakeHalfPair(b.mn[3 + d], b.mx[3 + d]);
#pragma unroll
    for (int d = 0; d < 3; ++d) w[13 + d] = BakeHalfPair(b.mn[10 + d], b.mx[10 + d]);
}
// (v - min) / (max - min) against the unrounded fp32 bounds (:613-637); the position too, whatever its format
GS_HD float BakeNorm(float v, float mn, float mx) { return (v - mn) / (mx - mn); }
GS_HD void BakeNormalise(BakeRec& o, const BakeBounds& b) {
    o.pos = { BakeNorm(o.pos.x, b.mn[0], b.mx[0]), BakeNorm(o.pos.y, b.mn[1], b.mx[1]), BakeNorm(o.pos.z, b.mn[2], b.mx[2]) };
    o.scale = { BakeNorm(o.scale.x, b.mn[3], b.mx[3]), BakeNorm(o.scale.y, b.mn[4], b.mx[4]), BakeNorm(o.scale.z, b.mn[5], b.mx[5]) };
    o.col = { BakeNorm(o.col.x, b.mn[6], b.mx[6]), BakeNorm(o.col.y, b.mn[7], b.mx[7]), BakeNorm(o.col.z, b.mn[8], b.mx[8]), BakeNorm(o.col.w, b.mn[9], b.mx[9]) };
#pragma unroll
    for (int k = 0; k < 15; ++k) {
#pragma unroll
        for (int d = 0; d < 3; ++d) o.sh[3 * k + d] = BakeNorm(o.sh[3 * k + d], b.mn[10 + d], b.mx[10 + d]);
    }
}
// truncating (uint)(v * (max + 0.5f)) of the encoders (:705-758).  The values it meets are normalised ones: inside [0, 1], or a NaN, which the
// importer's conversion leaves undefined -- 0 here, by a test
GS_HD uint32_t BakeQ(float v, float k) { const float p = v * k; return p == p ? (uint32_t)p : 0u; }
// EmitEncodedVector (:727-758, saturating): the words of one vector; the bytes used are vecStride(fmt)
GS_HD void BakeEmitVec(const V3& v, uint32_t fmt, uint32_t* w) {
    w[0] = f2u(v.x); w[1] = f2u(v.y); w[2] = f2u(v.z);
    if (fmt == 0) return;
    const float x = sat(v.x), y = sat(v.y), z = sat(v.z);
    w[1] = w[2] = 0u;
    if (fmt == 1) { w[0] = BakeQ(x, 65535.5f) | (BakeQ(y, 65535.5f) << 16); w[1] = BakeQ(z, 65535.5f); }
    else if (fmt == 2) w[0] = BakeQ(x, 2047.5f) | (BakeQ(y, 1023.5f) << 11) | (BakeQ(z, 2047.5f) << 21);
    else w[0] = BakeQ(x, 63.5f) | (BakeQ(y, 31.5f) << 6) | (BakeQ(z, 31.5f) << 11);
}
// the colour texel (:873-932): Float32x4 16 bytes, Float16x4 8, Norm8x4 4
GS_HD void BakeEmitColor(const V4& c, uint32_t fmt, uint32_t* w) {
    w[0] = f2u(c.x); w[1] = f2u(c.y); w[2] = f2u(c.z); w[3] = f2u(c.w);
    if (fmt == 0) return;
    w[2] = w[3] = 0u;
    if (fmt == 1) { w[0] = BakeHalfPair(c.x, c.y); w[1] = BakeHalfPair(c.z, c.w); }
    else { w[0] = BakeQ(sat(c.x), 255.5f) | (BakeQ(sat(c.y), 255.5f) << 8) | (BakeQ(sat(c.z), 255.5f) << 16) | (BakeQ(sat(c.w), 255.5f) << 24); w[1] = 0u; }
}
// the SH item (:934-1037; CreateSHDataJob does not saturate): all shStrideOf(fmt) / 4 words of it, the pad the importer leaves zero included.
// w: 48 words
GS_HD void BakeEmitSH(const float* sh, uint32_t fmt, uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 48; ++k) w[k] = 0u;
    if (fmt == 0) {
#pragma unroll
        for (int k = 0; k < 45; ++k) w[k] = f2u(sh[k]);
    } else if (fmt == 1) {
#pragma unroll
        for (int k = 0; k < 45; ++k) w[k >> 1] |= f32tof16(sh[k]) << ((k & 1) * 16);
    } else if (fmt == 2) {
#pragma unroll
        for (int j = 0; j < 15; ++j) w[j] = BakeQ(sh[3 * j], 2047.5f) | (BakeQ(sh[3 * j + 1], 1023.5f) << 11) | (BakeQ(sh[3 * j + 2], 2047.5f) << 21);
    } else {
#pragma unroll
        for (int j = 0; j < 15; ++j)
            w[j >> 1] |= ((BakeQ(sh[3 * j], 31.5f) | (BakeQ(sh[3 * j + 1], 63.5f) << 5) | (BakeQ(sh[3 * j + 2], 31.5f) << 11)) & 0xffffu) << ((j & 1) * 16);
    }
}
// the `other` record (:776-805): the rotation word, the scale, and in an asset with a Cluster* SH table the u16 index of the splat's table entry
// right behind the scale (:797-801).  w: 5 words; returns the bytes used: 4 + vecStride(scaleFmt), + 2 when clustered = 8, 10, 12 or 18
GS_HD bool shIsClustered(uint32_t shFormat) { return shFormat > 3u; }
// entries of the SH table: GS_SH_CLUSTER64K = 4 ... GS_SH_CLUSTER4K = 8; 0 for every other value (the importer's and the bake's one mapping)
GS_HD uint32_t shClusterCount(uint32_t shFormat) { return shFormat >= 4u && shFormat <= 8u ? 65536u >> (shFormat - 4u) : 0u; }
GS_HD uint32_t BakeEmitOther(uint32_t rot, const V3& scale, uint32_t scaleFmt, bool clustered, uint32_t shIndex, uint32_t* w) {
    w[0] = rot; w[4] = 0u;
    BakeEmitVec(scale, scaleFmt, w + 1);
    const uint32_t at = 4u + vecStride(scaleFmt);                  // even: the halfword at byte `at` is the low or the high half of word at / 4
    if (!clustered) return at;
    const uint32_t sh = (at & 2u) * 8u;
    w[at >> 2] = (w[at >> 2] & ~(0xffffu << sh)) | ((shIndex & 0xffffu) << sh);
    return at + 2u;
}
// one entry of the Cluster* SH table (ConvertSHClustersJob :443-474, SHTableItemFloat16): the 45 floats of a mean as fp16, the Float16 SH item's
// rounding, and 3 zero halfwords.  w: 24 words = 96 bytes
GS_HD void BakeEmitSHTableItem(const float* mean, uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 24; ++k) w[k] = 0u;
#pragma unroll
    for (int k = 0; k < 45; ++k) w[k >> 1] |= f32tof16(mean[k]) << ((k & 1) * 16);
}

// Morton code of a position inside the bounds of all splats (:362-429; MortonEncode3, GaussianUtils.cs:81-95): 21 bits per axis, z highest.  A
// component whose product is NaN -- a degenerate axis, max == min: 0 x inf -- is 0 by the test: the conversion of a NaN is undefined.
GS_HD uint64_t MortonPart1By2(uint64_t x) {
    x &= 0x1fffffull;
    x = (x ^ (x << 32)) & 0x1f00000000ffffull;
    x = (x ^ (x << 16)) & 0x1f0000ff0000ffull;
    x = (x ^ (x << 8)) & 0x100f00f00f00f00full;
    x = (x ^ (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x << 2)) & 0x1249249249249249ull;
    return x;
}
GS_HD uint32_t BakeMortonComponent(float p, float mn, float inv) {
    const float v = ((p - mn) * inv) * 2097151.0f;
    return v == v ? (uint32_t)v : 0u;
}
GS_HD uint64_t BakeMortonCode(const V3& p, const float* mn, const float* mx) {
    const float ix = 1.0f / (mx[0] - mn[0]), iy = 1.0f / (mx[1] - mn[1]), iz = 1.0f / (mx[2] - mn[2]);
    return (MortonPart1By2(BakeMortonComponent(p.z, mn[2], iz)) << 2) | (MortonPart1By2(BakeMortonComponent(p.y, mn[1], iy)) << 1) |
           MortonPart1By2(BakeMortonComponent(p.x, mn[0], ix));
}

// ---- import: raw splat arrays as the bake's source (gs_import.cpp:372-392, LinearizeData of GaussianFileReader.cs:211-233; kernels in
// gs_bake.hip) ------------------------------------------------------------------------------------------------------------------------
// The six arrays of gs_import_input, host or device memory
struct ImportSrc { const float* pos; const float* dc0; const float* sh; const float* opacity; const float* scale; const float* rot; };
// exp(x), the importer's exp_det: n = rint(x log2 e), r = x - n ln2 in two parts, the degree-5 polynomial of Cephes' expf, the scale by 2^n as an
// exponent splice.  fmin / fmax, nearbyintf and x + - only: the same bits on the host and on the device
GS_HD float ImportExpDet(float x) {
    x = fminf(fmaxf(x, -87.0f), 88.0f);
    const float n = nearbyintf(x * 1.44269504f);
    float r = x - n * 0.693359375f;
    r = r - n * -2.12194440e-4f;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    p = p * (r * r) + r;
    p = p + 1.0f;
    return p * u2f((uint32_t)((int)n + 127) << 23);
}
// LinearizeData on one splat: SH0ToColor, |exp(scale)|, Sigmoid(opacity), normalize(wxyz).yzwx packed smallest-three.  rot: (w, x, y, z) in,
// the packed three + index / 3 out
GS_HD void ImportLinearize(V3& dc0, V3& scale, float& opacity, V4& rot) {
    dc0 = { dc0.x * 0.2820948f + 0.5f, dc0.y * 0.2820948f + 0.5f, dc0.z * 0.2820948f + 0.5f };
    scale = { fabsf(ImportExpDet(scale.x)), fabsf(ImportExpDet(scale.y)), fabsf(ImportExpDet(scale.z)) };
    opacity = 1.0f / (1.0f + ImportExpDet(-opacity));
    const float len = sqrtf(((rot.x * rot.x + rot.y * rot.y) + rot.z * rot.z) + rot.w * rot.w);
    rot = PackSmallest3Rotation({ rot.y / len, rot.z / len, rot.w / len, rot.x / len });
}
// splat i of the raw arrays as the record the Bake* functions consume.  The rotation word is the importer's q(rot[k], 1023.5) | ... |
// q(rot[3], 3.5) << 30 of the four floats as they are (inside their field ranges: a premise with linearize = 0), not a re-pack of a quaternion
GS_HD void ImportRecord(const ImportSrc& in, uint32_t i, uint32_t linearize, BakeRec& o) {
    const uint64_t i3 = (uint64_t)i * 3u;
    o.pos = { in.pos[i3], in.pos[i3 + 1], in.pos[i3 + 2] };
    V3 dc0 = { in.dc0[i3], in.dc0[i3 + 1], in.dc0[i3 + 2] };
    o.scale = { in.scale[i3], in.scale[i3 + 1], in.scale[i3 + 2] };
    float opacity = in.opacity[i];
    const float* r = in.rot + (uint64_t)i * 4u;
    V4 rot = { r[0], r[1], r[2], r[3] };
    if (linearize) ImportLinearize(dc0, o.scale, opacity, rot);
    o.rot = BakeQ(rot.x, 1023.5f) | (BakeQ(rot.y, 1023.5f) << 10) | (BakeQ(rot.z, 1023.5f) << 20) | (BakeQ(rot.w, 3.5f) << 30);
    o.col = { dc0.x, dc0.y, dc0.z, opacity };
    const float* sh = in.sh + (uint64_t)i * 45u;
#pragma unroll
    for (int k = 0; k < 45; ++k) o.sh[k] = sh[k];
}

// ---- import from a file's own bytes (gs_import_file_to_asset; kernels in gs_bake.hip): the readers of gs_import.cpp restated per splat, so that
// the six arrays are never built.  Host and device from one text, as above -----------------------------------------------------------------------
// The vertex rows of a binary little-endian PLY as they lie in the file: row i at rows + i * stride, and where in a row each float property lies.
// off[]: x y z, f_dc_0..2, opacity, scale_0..2, rot_0..3, f_rest_0..44 (the 59 the importer reads), then nx ny nz (which it does not); -1 = the file
// has no float property of that name.  aligned: rows, stride and every offset that is read are multiples of 4 -- a field is then one dword load.
// inria: aligned, and the 59 offsets are those of the INRIA layout (x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3, what every
// trainer writes): the offsets are then compile-time constants, and the loads of neighbouring floats merge into wide ones as those of the six
// arrays do.  PlyRowLayout sets both
constexpr int kPlyOffsets = 62, kPlyOffsetsRead = 59;
constexpr int kPlyOffPos = 0, kPlyOffDc = 3, kPlyOffOpacity = 6, kPlyOffScale = 7, kPlyOffRot = 10, kPlyOffRest = 14, kPlyOffNormal = 59;
struct PlyRowSrc { const uint8_t* rows; uint32_t stride; uint32_t aligned, inria; int32_t off[kPlyOffsets]; };
// which float of an INRIA row entry k of the table is
GS_HD constexpr int PlyInriaFloat(int k) { return k < 3 ? k : (k < 6 ? k + 3 : (k == 6 ? 54 : (k < 14 ? k + 48 : k - 5))); }
GS_HD void PlyRowLayout(PlyRowSrc& s) {
    uint32_t low = s.stride | (uint32_t)(uintptr_t)s.rows;
    bool inria = true;
    for (int k = 0; k < kPlyOffsetsRead; ++k) {
        if (s.off[k] >= 0) low |= (uint32_t)s.off[k];
        inria = inria && s.off[k] == 4 * PlyInriaFloat(k);
    }
    s.aligned = (low & 3u) == 0u ? 1u : 0u;
    s.inria = s.aligned && inria ? 1u : 0u;
}
// the float property `k` of the row at `row`: 0 when absent (gs_ply_open's ld); else one dword, or four bytes assembled -- a row of odd stride
// starts at any address
GS_HD float PlyRowField(const PlyRowSrc& s, const uint8_t* row, int k) {
    const int32_t o = s.off[k];
    if (o < 0) return 0.0f;
    const uint8_t* p = row + o;
    if (s.aligned) return u2f(*(const uint32_t*)p);
    return u2f((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}
GS_HD V3 PlyRowPosition(const PlyRowSrc& s, uint32_t i) {
    const uint8_t* row = s.rows + (uint64_t)i * s.stride;
    if (s.inria) { const float* r = (const float*)row; return { r[0], r[1], r[2] }; }
    return { PlyRowField(s, row, kPlyOffPos), PlyRowField(s, row, kPlyOffPos + 1), PlyRowField(s, row, kPlyOffPos + 2) };
}
// row i as the record the Bake* functions consume: the 59 floats in the table's order, gs_ply_open's transpose (ReorderSHs: sh[j * 3 + c] =
// f_rest[c * 15 + j]), then ImportRecord with linearize = 1
GS_HD void PlyRowRecord(const PlyRowSrc& s, uint32_t i, BakeRec& o) {
    const uint8_t* row = s.rows + (uint64_t)i * s.stride;
    float f[kPlyOffsetsRead];
    if (s.inria) {
        const float* r = (const float*)row;
#pragma unroll
        for (int k = 0; k < kPlyOffsetsRead; ++k) f[k] = r[PlyInriaFloat(k)];
    } else {
#pragma unroll
        for (int k = 0; k < kPlyOffsetsRead; ++k) f[k] = PlyRowField(s, row, k);
    }
    o.pos = { f[kPlyOffPos], f[kPlyOffPos + 1], f[kPlyOffPos + 2] };
    V3 dc0 = { f[kPlyOffDc], f[kPlyOffDc + 1], f[kPlyOffDc + 2] };
    o.scale = { f[kPlyOffScale], f[kPlyOffScale + 1], f[kPlyOffScale + 2] };
    float opacity = f[kPlyOffOpacity];
    V4 rot = { f[kPlyOffRot], f[kPlyOffRot + 1], f[kPlyOffRot + 2], f[kPlyOffRot + 3] };
    ImportLinearize(dc0, o.scale, opacity, rot);
    o.rot = BakeQ(rot.x, 1023.5f) | (BakeQ(rot.y, 1023.5f) << 10) | (BakeQ(rot.z, 1023.5f) << 20) | (BakeQ(rot.w, 3.5f) << 30);
    o.col = { dc0.x, dc0.y, dc0.z, opacity };
#pragma unroll
    for (int j = 0; j < 15; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.sh[j * 3 + c] = f[kPlyOffRest + c * 15 + j];
    }
}

// The gunzipped stream of an SPZ file (SPZFileReader.cs:26-198): the 16-byte header, then for all n points the columns positions (3 x 24-bit fixed
// point), alphas, colours (3 bytes), scales (3), rotations (3), SH (shCoeffs x 3).  Header and sizes are checked by the host before a source is made
struct SpzSrc { const uint8_t* base; uint32_t n, shCoeffs, fractBits; };
GS_HD float SpzPositionComponent(const uint8_t* q, float fractScale) {
    int32_t fx = (int32_t)q[0] | ((int32_t)q[1] << 8) | ((int32_t)q[2] << 16);
    if (fx & 0x800000) fx |= (int32_t)0xff000000;                 // sign extension
    return (float)fx * fractScale;
}
GS_HD V3 SpzPosition(const SpzSrc& s, uint32_t i) {
    const float fractScale = 1.0f / (float)(1 << s.fractBits);
    const uint8_t* q = s.base + 16u + (uint64_t)i * 9u;
    return { SpzPositionComponent(q, fractScale), SpzPositionComponent(q + 3, fractScale), SpzPositionComponent(q + 6, fractScale) };
}
GS_HD float SpzScale(uint8_t b) { return fabsf(ImportExpDet((float)b / 16.0f - 10.0f)); }                        // LinearScale
GS_HD float SpzColor(uint8_t b) { return (((float)b / 255.0f - 0.5f) / 0.15f) * 0.2820948f + 0.5f; }             // SH0ToColor
// point i as the record the Bake* functions consume: spz_open_impl's per-splat loop (UnpackDataJob :141-205), operation for operation, then what
// ImportRecord does with linearize = 0.  The SH quirk is kept: fifteen coefficients from i * 3 * shCoeffs whatever the level, bytes past the array
// reading as 128
GS_HD void SpzRecord(const SpzSrc& s, uint32_t i, BakeRec& o) {
    const uint64_t N = s.n, i3 = (uint64_t)i * 3u;
    const uint8_t* alpha = s.base + 16u + N * 9u;
    const uint8_t* col = alpha + N;
    const uint8_t* scale = col + N * 3u;
    const uint8_t* rotb = scale + N * 3u;
    const uint8_t* sh = rotb + N * 3u;
    o.pos = SpzPosition(s, i);
    o.scale = { SpzScale(scale[i3]), SpzScale(scale[i3 + 1]), SpzScale(scale[i3 + 2]) };
    o.col = { SpzColor(col[i3]), SpzColor(col[i3 + 1]), SpzColor(col[i3 + 2]), (float)alpha[i] / 255.0f };
    const float qx = (float)rotb[i3] * (1.0f / 127.5f) - 1.0f, qy = (float)rotb[i3 + 1] * (1.0f / 127.5f) - 1.0f, qz = (float)rotb[i3 + 2] * (1.0f / 127.5f) - 1.0f;
    const float sq = (qx * qx + qy * qy) + qz * qz;
    const float qw = sqrtf(fmaxf(0.0f, 1.0f - sq));
    const float inv = 1.0f / sqrtf(((qx * qx + qy * qy) + qz * qz) + qw * qw);            // math.normalize
    const V4 rot = PackSmallest3Rotation({ qx * inv, qy * inv, qz * inv, qw * inv });
    o.rot = BakeQ(rot.x, 1023.5f) | (BakeQ(rot.y, 1023.5f) << 10) | (BakeQ(rot.z, 1023.5f) << 20) | (BakeQ(rot.w, 3.5f) << 30);
    const uint64_t shLen = N * 3u * s.shCoeffs, first = i3 * s.shCoeffs;
#pragma unroll
    for (int k = 0; k < 45; ++k) {
        const uint64_t at = first + (uint64_t)k;
        const float bv = at < shLen ? (float)sh[at] : 128.0f;
        o.sh[k] = (bv - 128.0f) / 128.0f;
    }
}

// ---- BC7 mode-6 colour blocks (bc7_encode_mode6 of gs_import.cpp, operation for operation): the colour texture of the VeryLow preset ------------
// Three steps, so that one thread can own a block (BC7EncodeMode6) or sixteen lanes can, each with its texel: the per-block endpoints from
// the channel minima / maxima, the per-texel index, the per-block packing of the sixteen indices.
struct BC7Block { int q0[4], q1[4], p0, p1; float e0[4], axis[4], den; };
// a texel as the encoder sees it: clamp(v, 0, 1) x 255
GS_HD void BC7Texel(const V4& c, float* px) { px[0] = sat(c.x) * 255.0f; px[1] = sat(c.y) * 255.0f; px[2] = sat(c.z) * 255.0f; px[3] = sat(c.w) * 255.0f; }
// the two-p-bit endpoint quantiser: floor((v - p) / 2 + 0.5) clamped to 0..127, the squared error summed left to right, p = 1 only when strictly better
GS_HD void BC7QuantEndpoint(const float* v, int* q, int& pbit) {
    float berr = 0.0f;
    pbit = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float qq[4], err = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            qq[c] = fminf(fmaxf(floorf((v[c] - (float)p) / 2.0f + 0.5f), 0.0f), 127.0f);
            const float d = (qq[c] * 2.0f + (float)p) - v[c];
            const float d2 = d * d;
            err = c == 0 ? d2 : err + d2;
        }
        if (p == 0 || err < berr) {
            berr = err; pbit = p;
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = (int)qq[c];
        }
    }
}
GS_HD void BC7Endpoints(const float* lo, const float* hi, BC7Block& b) {
    BC7QuantEndpoint(lo, b.q0, b.p0);
    BC7QuantEndpoint(hi, b.q1, b.p1);
    b.den = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        b.e0[c] = (float)(b.q0[c] * 2 + b.p0);
        b.axis[c] = (float)(b.q1[c] * 2 + b.p1) - b.e0[c];
        const float a2 = b.axis[c] * b.axis[c];
        b.den = c == 0 ? a2 : b.den + a2;
    }
}
// the nearest of the 16 mode-6 weights to the texel's projection on the endpoint axis: the first minimum wins
GS_HD uint32_t BC7TexelIndex(const BC7Block& b, const float* px) {
    float num = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) { const float m = (px[c] - b.e0[c]) * b.axis[c]; num = c == 0 ? m : num + m; }
    const float tt = num / fmaxf(b.den, 1.0e-6f);
    uint32_t best = 0;
    float bd = fabsf(tt - 0.0f);
#pragma unroll
    for (uint32_t k = 1; k < 16u; ++k) {
        const float w = (float)((k * 64u + 7u) / 15u) / 64.0f;      // 0 4 9 13 17 21 26 30 34 38 43 47 51 55 60 64, over 64
        const float d = fabsf(tt - w);
        if (d < bd) { bd = d; best = k; }
    }
    return best;
}
// the 128 bits of the block; nib: the index of texel t (row-major in the block) in bits 4 t .. 4 t + 3.  Texel 0 is the anchor: its index must
// have the top bit clear, so with an index >= 8 there every index is flipped and the endpoints change places
GS_HD void BC7Pack(const BC7Block& b, uint64_t nib, uint32_t* w) {
    const bool flip = (nib & 8u) != 0u;
    if (flip) nib = ~nib;
    uint64_t lo = 1ull << 6;
    uint32_t at = 7;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        lo |= (uint64_t)(uint32_t)(flip ? b.q1[c] : b.q0[c]) << at; at += 7;
        lo |= (uint64_t)(uint32_t)(flip ? b.q0[c] : b.q1[c]) << at; at += 7;
    }
    lo |= (uint64_t)(uint32_t)(flip ? b.p1 : b.p0) << 63;
    const uint64_t hi = (uint64_t)(uint32_t)(flip ? b.p0 : b.p1) | ((nib & 7ull) << 1) | (nib & ~0xfull);
    w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = (uint32_t)hi; w[3] = (uint32_t)(hi >> 32);
}
// one block on one thread: px = 16 texels (row-major) x RGBA as BC7Texel gives them
GS_HD void BC7EncodeMode6(const float (*px)[4], uint32_t* w) {
    float lo[4], hi[4];
    for (int c = 0; c < 4; ++c) { lo[c] = hi[c] = px[0][c]; for (int t = 1; t < 16; ++t) { lo[c] = fminf(lo[c], px[t][c]); hi[c] = fmaxf(hi[c], px[t][c]); } }
    BC7Block b;
    BC7Endpoints(lo, hi, b);
    uint64_t nib = 0;
    for (int t = 0; t < 16; ++t) nib |= (uint64_t)BC7TexelIndex(b, px[t]) << (4 * t);
    BC7Pack(b, nib, w);
}
// where a splat's texel lies among the BC7 blocks: destination records 16 b .. 16 b + 15 of a chunk are one 4 x 4 block (SplatIndexToPixelIndex
// de-interleaves the low 8 bits), and record bits 0, 2, 1, 3 are the bits of the texel's row-major place inside it
GS_HD uint32_t BC7TexelOfLane(uint32_t i) { return (i & 9u) | ((i & 4u) >> 1) | ((i & 2u) << 1); }
GS_HD uint64_t BC7BlockOfSplat(uint32_t i) {
    uint32_t px, py;
    SplatIndexToPixelIndex(i, px, py);
    return (uint64_t)(py >> 2) * 512u + (px >> 2);
}

// One destination chunk on one thread: the records of its cnt <= 256 splats (already linear) to the bytes of the five blobs at splat index
// first + k -- what the kernel's workgroup does with one lane per splat, and what the host harness of the tests runs as it stands.  A Cluster* SH
// target (shIndex: the table index of every record, in destination order) writes the index into `other` and no SH item: the table is the caller's.
GS_HD void BakeStoreBytes(uint8_t* dst, const uint32_t* w, uint32_t bytes) {
    for (uint32_t k = 0; k < bytes; ++k) dst[k] = (uint8_t)(w[k >> 2] >> ((k & 3u) * 8u));
}
GS_HD void BakeEncodeChunkSerial(BakeRec* rec, uint32_t cnt, uint32_t first, const BakeFormats& f, uint8_t* pos, uint8_t* other, uint8_t* color,
                                 uint8_t* sh, uint8_t* chunk, const uint32_t* shIndex = nullptr) {
    BakeBounds b;
    if (f.chunked) {
        BakeBoundsEmpty(b);
        for (uint32_t k = 0; k < cnt; ++k) { BakeChunkSpace(rec[k]); BakeBounds one; BakeBoundsOf(rec[k], one); BakeBoundsMerge(b, one); }
        BakeBoundsWiden(b);
        uint32_t w[16];
        BakeChunkWords(b, w);
        BakeStoreBytes(chunk + (uint64_t)(first >> 8) * 64u, w, 64u);
    }
    const bool clustered = shIsClustered(f.sh);
    const uint32_t posSz = vecStride(f.pos), colSz = f.color == 0 ? 16u : (f.color == 1 ? 8u : 4u), shSz = shStrideOf(f.sh);
    for (uint32_t k = 0; k < cnt; ++k) {
        BakeRec& o = rec[k];
        if (f.chunked) BakeNormalise(o, b);
        const uint64_t i = (uint64_t)first + k;
        uint32_t w[48];
        BakeEmitVec(o.pos, f.pos, w);
        BakeStoreBytes(pos + i * posSz, w, posSz);
        const uint32_t othSz = BakeEmitOther(o.rot, o.scale, f.scale, clustered, clustered ? shIndex[i] : 0u, w);
        BakeStoreBytes(other + i * othSz, w, othSz);
        uint32_t px, py;
        SplatIndexToPixelIndex((uint32_t)i, px, py);
        BakeEmitColor(o.col, f.color, w);
        if (f.color != 3u) BakeStoreBytes(color + ((uint64_t)py * 2048u + px) * colSz, w, colSz);
        if (clustered) continue;
        BakeEmitSH(o.sh, f.sh, w);
        BakeStoreBytes(sh + i * shSz, w, shSz);
    }
    if (f.color != 3u) return;
    for (uint32_t blk = 0; blk < 16u; ++blk) {                     // a BC7 colour target: the chunk's tile is sixteen blocks, a record past cnt a zero texel
        float px[16][4];
        for (uint32_t l = 0; l < 16u; ++l) {
            const uint32_t k = blk * 16u + l;
            const V4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
            BC7Texel(k < cnt ? rec[k].col : zero, px[BC7TexelOfLane(l)]);
        }
        uint32_t w[4];
        BC7EncodeMode6(px, w);
        BakeStoreBytes(color + BC7BlockOfSplat(first + blk * 16u) * 16u, w, 16u);
    }
}

// ---- the edit history's compaction (gs_renderer_edit_checkpoint; kernels in gs_edit.hip) ----------------------------
// A checkpoint journals the records of the splats selected NOW, in index order: splat s of 256-splat block b goes to journal slot
// base[b] + HistRank(m, s & 255), base = the exclusive prefix of HistBlockCount over the blocks.  Bits of the last word at indices >= n (select-all
// and invert set them) name no splat and are masked off first.
constexpr uint32_t kHistBlock = 256;                               // splats per block: eight selection words
// selection word `w` (splats 32 w .. 32 w + 31) of a renderer of n splats without the bits at indices >= n
GS_HD uint32_t HistMaskedWord(uint32_t word, uint32_t w, uint32_t n) {
    const uint32_t first = w * 32u;
    if (first >= n) return 0u;
    const uint32_t left = n - first;
    return left >= 32u ? word : (word & ((1u << left) - 1u));
}
// the eight masked words of block b (a word index >= nWords reads as zero)
GS_HD void HistBlockWords(const uint32_t* sel, uint32_t nWords, uint32_t n, uint32_t b, uint32_t m[8]) {
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t w = b * 8u + j;
        m[j] = w < nWords ? HistMaskedWord(sel[w], w, n) : 0u;
    }
}
// selected splats of the block
GS_HD uint32_t HistBlockCount(const uint32_t m[8]) {
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) c += (uint32_t)__builtin_popcount(m[j]);
    return c;
}
// selected splats of the block below splat t (0 .. 255) of it: the splat's journal slot inside the block if it is selected itself
GS_HD uint32_t HistRank(const uint32_t m[8], uint32_t t) {
    const uint32_t wj = t >> 5, below = (1u << (t & 31u)) - 1u;
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j)                              // (no m[wj]: a register array is never indexed by a variable)
        r += (uint32_t)__builtin_popcount(m[j] & (j < wj ? ~0u : (j == wj ? below : 0u)));
    return r;
}

// ---- fixed-radius neighbour counts on a grid (gs_renderer_edit_neighbour_counts / _select_sparse; kernels in gs_neighbours.hip) ----
// The predicate is fp32, operation by operation; the grid only decides which pairs are looked at, in fp64: a cell is radius (1 + 2^-10) wide, so two
// splats the predicate joins lie at most one cell apart on every axis (the argument: section 4.17).  The listed splats -- alive, finite position -- are
// sorted by cell key with x the lowest field: the cells (x-1 .. x+1, y, z) are one contiguous run of the sorted array, and a splat visits nine such runs.
constexpr uint32_t kNeighbourCellMax = (1u << 21) - 1u;            // 21 bits per axis
struct alignas(16) NeighbourRec { float x, y, z; uint32_t idx; };  // a listed splat in sorted order: its position and its index in the renderer

// every comparison with NaN is false and inf - inf is NaN: a splat with a non-finite component is never listed
GS_HD bool NeighbourFinite(V3 p) {
    return (f2u(p.x) & 0x7f800000u) != 0x7f800000u && (f2u(p.y) & 0x7f800000u) != 0x7f800000u && (f2u(p.z) & 0x7f800000u) != 0x7f800000u;
}
GS_HD double NeighbourCellEdge(float radius) { return (double)radius * 1.0009765625; }      // 1 + 2^-10
// p, origin finite, origin <= p, h > 0: the quotient is >= 0 and never NaN; the clamp is monotone
GS_HD uint32_t NeighbourCellCoord(float p, float origin, double h) {
    const double c = floor(((double)p - (double)origin) / h);
    return c >= (double)kNeighbourCellMax ? kNeighbourCellMax : (c > 0.0 ? (uint32_t)c : 0u);
}
GS_HD unsigned long long NeighbourKey(uint32_t cx, uint32_t cy, uint32_t cz) {
    return (unsigned long long)cx | ((unsigned long long)cy << 21) | ((unsigned long long)cz << 42);
}
GS_HD unsigned long long NeighbourKeyOf(V3 p, const float* origin, double h) {
    return NeighbourKey(NeighbourCellCoord(p.x, origin[0], h), NeighbourCellCoord(p.y, origin[1], h), NeighbourCellCoord(p.z, origin[2], h));
}
// N(i, j): d2 = (dx dx + dy dy) + dz dz <= r2, the boundary included
GS_HD bool NeighbourTest(const NeighbourRec& i, const NeighbourRec& j, float r2) {
    const float dx = j.x - i.x, dy = j.y - i.y, dz = j.z - i.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= r2;
}
// the keys of the first and the last cell of the run (cx-1 .. cx+1, cy + dy, cz + dz); false: that row of cells lies outside the grid and is SKIPPED
// (clamped, it would coincide with a row already visited and its splats would be counted twice).  On x, leaving out the cells outside is the clip.
GS_HD bool NeighbourRun(unsigned long long key, int dy, int dz, unsigned long long& first, unsigned long long& last) {
    const uint32_t cx = (uint32_t)key & kNeighbourCellMax, cy = (uint32_t)(key >> 21) & kNeighbourCellMax, cz = (uint32_t)(key >> 42) & kNeighbourCellMax;
    const int y = (int)cy + dy, z = (int)cz + dz;
    if (y < 0 || y > (int)kNeighbourCellMax || z < 0 || z > (int)kNeighbourCellMax) return false;
    first = NeighbourKey(cx > 0u ? cx - 1u : 0u, (uint32_t)y, (uint32_t)z);
    last = NeighbourKey(cx < kNeighbourCellMax ? cx + 1u : kNeighbourCellMax, (uint32_t)y, (uint32_t)z);
    return true;
}
// first index in [lo, hi) whose key is >= k (orEqual) / > k (!orEqual); hi if there is none
GS_HD uint32_t NeighbourBound(const unsigned long long* keys, uint32_t lo, uint32_t hi, unsigned long long k, bool orEqual) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const unsigned long long v = keys[mid];
        if (orEqual ? v < k : v <= k) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// first index in [a, m) whose key is > last, a being where the run starts: a run is a few splats long -- most are empty -- so the end is looked for
// from a in doubling steps and only the last step is bisected (an empty run costs one load, not log2 m: the count kernel took 0.79 of its time at
// 6.1 M splats)
GS_HD uint32_t NeighbourRunEnd(const unsigned long long* keys, uint32_t a, uint32_t m, unsigned long long last) {
    uint32_t lo = a, hi = a, step = 1u;
    while (hi < m && keys[hi] <= last) { lo = hi + 1u; hi += step; step <<= 1; }       // every key below lo is <= last; keys[hi] > last, or hi >= m
    return NeighbourBound(keys, lo, hi < m ? hi : m, last, false);
}
// min(count(i), limit) of the listed splat at sorted position i among the m listed ones: nine runs, each found by a binary search for its start and
// NeighbourRunEnd and walked in order; the walk stops at `limit` and never counts the splat itself.  tests: += the predicates evaluated (a statistic)
GS_HD uint32_t NeighbourCount(const unsigned long long* keys, const NeighbourRec* recs, uint32_t m, uint32_t i, float r2, uint32_t limit, uint32_t& tests) {
    if (limit == 0u) return 0u;
    const NeighbourRec me = recs[i];
    const unsigned long long key = keys[i];
    uint32_t count = 0u;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            unsigned long long first, last;
            if (!NeighbourRun(key, dy, dz, first, last)) continue;
            const uint32_t a = NeighbourBound(keys, 0u, m, first, true);
            const uint32_t b = NeighbourRunEnd(keys, a, m, last);
            for (uint32_t j = a; j < b; ++j) {
                if (j == i) continue;
                ++tests;
                if (NeighbourTest(me, recs[j], r2) && ++count == limit) return count;
            }
        }
    return count;
}
// edge(j) for every sorted position j < i with N(i, j): the edges of the neighbour graph, each handed out once, at its later end (N is symmetric in
// fp32: xj - xi is exactly -(xi - xj)).  The nine runs of NeighbourCount, rows outside the grid skipped; the sorted keys ascend, so a run that starts
// at or beyond i holds no j < i and a run is walked up to i at most
template <class Edge>
GS_HD void NeighbourForEach(const unsigned long long* keys, const NeighbourRec* recs, uint32_t m, uint32_t i, float r2, Edge&& edge) {
    const NeighbourRec me = recs[i];
    const unsigned long long key = keys[i];
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            unsigned long long first, last;
            if (!NeighbourRun(key, dy, dz, first, last)) continue;
            if (first > key) continue;                             // every key of the run is above this splat's: it lies behind i
            const uint32_t a = NeighbourBound(keys, 0u, m, first, true);
            if (a >= i) continue;
            const uint32_t b = NeighbourRunEnd(keys, a, m, last);
            for (uint32_t j = a; j < b; ++j) {
                if (j >= i) break;
                if (NeighbourTest(me, recs[j], r2)) edge(j);
            }
        }
}

// ---- selection by attribute (gs_renderer_edit_attribute_* / _select_range; kernels in gs_attributes.hip) -----------------------
// One fp32 value per splat from LoadSplatData's decoded fields, operation by operation, nothing fused; tests/attribute_host_harness.cpp runs every
// function below on the host.  The attributes fall into four CLASSES by the bytes they need: a kernel is built per class and loads nothing else.
enum { kAttrOpacity = 0, kAttrScaleMax = 1, kAttrScaleMin = 2, kAttrVolume = 3, kAttrPosX = 4, kAttrPosY = 5, kAttrPosZ = 6, kAttrDist2 = 7,
       kAttrColorR = 8, kAttrColorG = 9, kAttrColorB = 10, kAttrLuma = 11, kAttrCount = 12 };      // gs_splat_attribute
enum { kAttrClassPos = 0, kAttrClassScale = 1, kAttrClassOpacity = 2, kAttrClassColor = 3 };
GS_HD int AttributeClass(int attr) {
    return attr == kAttrOpacity ? kAttrClassOpacity : (attr <= kAttrVolume ? kAttrClassScale : (attr <= kAttrDist2 ? kAttrClassPos : kAttrClassColor));
}
// the partial forms of LoadSplatDataFull the classes read: the scale alone (the other blob and the chunk header; no colour texel) ...
GS_HD V3 LoadSplatScale(const AssetView& a, uint32_t idx, uint32_t ci) {
    uint32_t otherStride = 4 + vecStride(a.scaleFmt);
    if (a.shFmt > 3) otherStride += 2;
    V3 scale = LoadVec(a.other, (uint64_t)idx * otherStride + 4, a.scaleFmt);
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        scale.x = lerpf(f16tof32(ld32a(c, 40)), f16tof32(ld32a(c, 40) >> 16), scale.x);
        scale.y = lerpf(f16tof32(ld32a(c, 44)), f16tof32(ld32a(c, 44) >> 16), scale.y);
        scale.z = lerpf(f16tof32(ld32a(c, 48)), f16tof32(ld32a(c, 48) >> 16), scale.z);
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
        scale.x *= scale.x; scale.y *= scale.y; scale.z *= scale.z;
    }
    return scale;
}
// ... and the opacity alone (the colour texel and the chunk header; neither the other blob nor SH)
GS_HD float LoadSplatOpacity(const AssetView& a, uint32_t idx, uint32_t ci) {
    float o = LoadColorTexel(a, idx).w;
    if (ci < a.chunkCount) {
        const uint8_t* c = a.chunk + (uint64_t)ci * 64;
        o = InvSquareCentered01(lerpf(f16tof32(ld32a(c, 12)), f16tof32(ld32a(c, 12) >> 16), o));
    }
    return o;
}
// fmaxf / fminf with the one case the C standard leaves open pinned: of +0 and -0 the FIRST operand is returned.  A NaN operand is ignored; NaN if both are
GS_HD float AttributeMax(float a, float b) { return (a >= b || b != b) ? a : b; }
GS_HD float AttributeMin(float a, float b) { return (a <= b || b != b) ? a : b; }
GS_HD float AttributeOfScale(int attr, V3 s) {
    if (attr == kAttrScaleMax) return AttributeMax(AttributeMax(s.x, s.y), s.z);
    if (attr == kAttrScaleMin) return AttributeMin(AttributeMin(s.x, s.y), s.z);
    return (s.x * s.y) * s.z;
}
GS_HD float AttributeOfPos(int attr, V3 p, V3 q) {                // q: the point of kAttrDist2 (N(i, j)'s d2)
    if (attr == kAttrPosX) return p.x;
    if (attr == kAttrPosY) return p.y;
    if (attr == kAttrPosZ) return p.z;
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}
GS_HD float AttributeOfColor(int attr, V3 c) {
    if (attr == kAttrColorR) return c.x;
    if (attr == kAttrColorG) return c.y;
    if (attr == kAttrColorB) return c.z;
    return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z;
}
// value(i, attr) of a splat whose position the caller has loaded (or not: only the position class reads it)
GS_HD float AttributeValue(const AssetView& a, int attr, uint32_t idx, uint32_t ci, V3 pos, V3 q) {
    const int cls = AttributeClass(attr);
    if (cls == kAttrClassPos) return AttributeOfPos(attr, pos, q);
    if (cls == kAttrClassScale) return AttributeOfScale(attr, LoadSplatScale(a, idx, ci));
    if (cls == kAttrClassOpacity) return LoadSplatOpacity(a, idx, ci);
    return AttributeOfColor(attr, LoadSplatBaseColor(a, idx));
}
GS_HD bool AttributeIsNaN(float v) { return v != v; }
GS_HD bool AttributeInRange(float v, float lo, float hi) { return lo <= v && v <= hi; }          // false for a NaN, and for every v when lo > hi
// the word of the bins + 3 histogram words a value is counted in: s = (float) bins / (hi - lo), computed once by the host
GS_HD uint32_t AttributeBin(float v, float lo, float hi, float s, uint32_t bins) {
    if (v != v) return bins + 2u;
    if (v < lo) return bins;
    if (v > hi) return bins + 1u;
    const float t = (v - lo) * s;
    const uint32_t b = (uint32_t)t;
    return b < bins - 1u ? b : bins - 1u;
}
GS_HD float SortableUintToFloat(uint32_t u) { return u2f((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }      // FloatToSortableUint's inverse

} // namespace gsm
