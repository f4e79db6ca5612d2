// What the units of the layer-GEMM family share (gemm.hip holds the overview and the map of the units): the operand producers,
// LDS tile staging and the MFMA tile, the pool / statistics epilogues, the split-bf16 arithmetic, the diagnostic macros, and the
// declarations of the option block and of the host functions that cross the units.
#pragma once
#include "common.hpp"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ceil(a / b) on the device (the layer GEMMs are its only callers).  `used` keeps it out of the per-unit internalisation: the dX tile
// kernels call it with b = KT, the dW kernels with b = gridDim.y, and a unit that holds only the former would have the constant
// divisor propagated into the helper before it is inlined -- the sixteen gemm_dx_kernel instantiations then compile differently
// (eight of them with more scratch) from the code they were measured as.
__device__ __forceinline__ __attribute__((used)) int gad_cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// cache policy of the streaming kernels' big output stores (buffer-store aux bits: 0 plain, 2 nt, 16 sc1 = write-through)
#ifndef GAD_STREAM_STORE_AUX
#define GAD_STREAM_STORE_AUX 0
#endif

#define KT 32   // reduction tile

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4sel(bool c, float4 a, float4 b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

typedef unsigned gad_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    const gad_u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0);
    return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
}
__device__ __forceinline__ float buf_ld(__amdgpu_buffer_rsrc_t r, int vo, int so) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
}
// buffer descriptors address 32-bit UNSIGNED byte offsets: a row tensor may reach 2 GiB (the host-side route predicates bound
// rows x pitch x 4 by 2^31 inclusive, fits_i32_bytes) -- record counts are formed in unsigned arithmetic
#define GAD_BUF_MAX ((int)0x80000000u)
__device__ __forceinline__ int gad_nbytes(int rows, int row_bytes) { return (int)((unsigned)rows * (unsigned)row_bytes); }

// ------------------------------------------------------------------------------------------------
// operand producers.  Every producer is split in two so that global loads overlap the MFMAs:
//   *_raw    issues the 16-byte loads of the NEXT tile into registers (no arithmetic on them),
//   *_finish runs after the current tile's MFMAs, right before the LDS store: BatchNorm affine /
//            ReLU / BatchNorm-backward with the per-channel vectors read from LDS.
// ------------------------------------------------------------------------------------------------
#define VMAX 1024            // max channels of one layer side (per-channel vectors staged in LDS)

struct XSrc {   // how a layer's INPUT row r, column c is produced (gad_gemm_fwd_args subset)
    int mode;
    const float* zin; int zin_pitch; int c_in;
    const float* scale; const float* shift; int relu;
    const float* extra; int ones_col;
    const float* src_xyz; const float* ctr_xyz; const float* feat; int feat_c;
    const float* action; int act_c; int gps;
    const int32_t* row_pt; const int32_t* row_grp;
    int affine;          // ACT input: a per-channel affine (scale / shift) is applied
    const float* pre_W; int pre_Kp;   // mode 2: the ACT input is RECOMPUTED from the gathered first layer (its packed weights)
    gad_bn_fin bn;       // input layer's BatchNorm finalised in this launch's prologue (bn.stat_sum == NULL: scale / shift as given)
};

static XSrc make_xsrc(const gad_gemm_fwd_args& a) {
    XSrc x;
    x.mode = a.mode; x.zin = a.zin; x.zin_pitch = a.zin_pitch; x.c_in = a.c_in;
    x.scale = a.scale; x.shift = a.shift; x.relu = a.relu; x.extra = a.extra; x.ones_col = a.ones_col;
    x.src_xyz = a.src_xyz; x.ctr_xyz = a.ctr_xyz; x.feat = a.feat; x.feat_c = a.feat_c;
    x.action = a.action; x.act_c = a.act_c; x.gps = a.grp_per_sample > 0 ? a.grp_per_sample : 1;
    x.row_pt = a.row_pt; x.row_grp = a.row_grp;
    x.affine = (x.scale && x.shift) ? 1 : 0;
    x.pre_W = a.pre_W; x.pre_Kp = a.pre_Kp;
    x.bn.stat_sum = a.in_stat_sum; x.bn.stat_sq = a.in_stat_sq; x.bn.stat_stride = a.in_stat_stride; x.bn.count = a.in_count;
    x.bn.gamma = a.in_gamma; x.bn.beta = a.in_beta; x.bn.eps = a.in_eps; x.bn.momentum = a.in_momentum;
    x.bn.running_mean = a.in_running_mean; x.bn.running_var = a.in_running_var;
    x.bn.scale = const_cast<float*>(a.scale); x.bn.shift = const_cast<float*>(a.shift); x.bn.mean = a.in_mean; x.bn.istd = a.in_istd;
    return x;
}

// per-channel affine of an ACT input -> LDS
template <int NT>
__device__ __forceinline__ void stage_affine(float* sv, float* tv, const XSrc& x, int off, int n) {
    for (int i = threadIdx.x; i < n; i += NT) { sv[i] = x.scale[off + i]; tv[i] = x.shift[off + i]; }
}

// diagnostic build (-DGAD_X_PHASES=1, tools/ubench_phases.py): the streaming forward kernel writes each wavefront's cycles per
// phase (wait + prefetch | MFMA loop | epilogue) into the launch's timing slot instead of the start / end stamps
#ifdef GAD_X_PHASES
#define GAD_PH_STAMP(t) t = (long long)__builtin_readcyclecounter()
#else
#define GAD_PH_STAMP(t)
#endif
// diagnostic build (-DGAD_W_PHASES, tools/ubench_wphases.py): the wide-tile forward / dX kernels write, per workgroup, the wall
// clock (100 MHz) at the end of each part of their first row tile -- prologue | first tile staged | K loop | stores + statistics |
// column atomics -- into the upper half of the launch's timing slot (entries 8192 + workgroup)
#ifdef GAD_W_PHASES
#define GAD_WPH_DECL long long wph_[6] = {0, 0, 0, 0, 0, 0}; wph_[0] = (long long)wall_clock64()
#define GAD_WPH(i) do { if (wph_[i] == 0) wph_[i] = (long long)wall_clock64(); } while (0)
#define GAD_WPH_STORE(ts)                                                                                                     \
    do {                                                                                                                      \
        unsigned long long* q_ = reinterpret_cast<unsigned long long*>(reinterpret_cast<size_t>(ts) & ~(size_t)7);            \
        const unsigned blk_ = blockIdx.x + gridDim.x * blockIdx.y;                                                            \
        if (q_ && threadIdx.x == 0 && blk_ < 4096) {                                                                          \
            auto c_ = [&](int i) { const long long d_ = wph_[i] ? wph_[i] - wph_[0] : 0; return (unsigned long long)(d_ > 65535 ? 65535 : d_); }; \
            q_[2 * (8192 + blk_)] = (unsigned long long)wph_[0];                                                              \
            q_[2 * (8192 + blk_) + 1] = c_(1) | (c_(2) << 16) | (c_(3) << 32) | (c_(4) << 48);                                \
            q_[2 * (12288 + blk_)] = c_(5);                                                                                    \
        }                                                                                                                     \
    } while (0)
// ... and, summed over the K-tiles of the first row tile, every wavefront's shader cycles in: fragments + MFMAs issued | next tile
// staged + loads issued | barrier wait (entries 4096 + 8 * workgroup + wavefront: {mfma << 32 | stage, barrier})
#define GAD_WKL_DECL long long wkl_[4] = {0, 0, 0, 0}; long long wkt_ = 0, wkp_ = 0
#define GAD_WKL(i)                                                                   \
    do {                                                                             \
        wkt_ = (long long)__builtin_readcyclecounter();                              \
        if (i > 0) wkl_[i] += wkt_ - wkp_;                                           \
        wkp_ = wkt_;                                                                 \
    } while (0)
#define GAD_WKL_STORE(ts)                                                                                                     \
    do {                                                                                                                      \
        unsigned long long* q_ = reinterpret_cast<unsigned long long*>(reinterpret_cast<size_t>(ts) & ~(size_t)7);            \
        const unsigned blk_ = blockIdx.x + gridDim.x * blockIdx.y;                                                            \
        if (q_ && (threadIdx.x & 63) == 0 && blk_ < 512) {                                                                    \
            const unsigned e_ = 4096 + 8 * blk_ + (threadIdx.x >> 6);                                                         \
            q_[2 * e_] = ((unsigned long long)wkl_[1] << 32) | (unsigned long long)(wkl_[2] & 0xffffffffu);                   \
            q_[2 * e_ + 1] = (unsigned long long)wkl_[3];                                                                     \
        }                                                                                                                     \
    } while (0)
#else
#define GAD_WPH_DECL
#define GAD_WPH(i)
#define GAD_WPH_STORE(ts)
#define GAD_WKL_DECL
#define GAD_WKL(i)
#define GAD_WKL_STORE(ts)
#endif
struct XRaw { float4 a; float4 s; };     // a: the 16 raw bytes; s: special columns (tail tiles only)

// number of leading "bulk" columns served by aligned 16-byte loads
__device__ __forceinline__ int x_bulk(const XSrc& x) { return x.mode == 0 ? x.c_in : x.feat_c; }

// ACT input: columns [0,c_in) = act(scale*z+shift) of the previous layer's raw output (c_in % 4 == 0),
//            column c_in = extra[r] (optional), column ones_col = 1, everything else 0.
// GATHER input (packed order, features first): [feat[pt] (feat_c) | src_xyz[pt]-ctr_xyz[grp] (3) |
//            action[grp/gps] (act_c) | 0..].
// `tail` (wave-uniform): this K-tile reaches beyond the bulk columns.  `pt`: point index of the row.
template <int XM>
__device__ __forceinline__ XRaw x_raw(const XSrc& x, int r, bool valid, int zoff, int c, bool tail, int pt, int grp_pre = -1) {
    XRaw o;
    o.s = f4zero();
    const int rr = valid ? r : 0;
    if (XM == 0) {
        const int cc = c < x.c_in ? c : x.c_in - 4;
        o.a = ldg4(x.zin + (size_t)rr * x.zin_pitch + zoff + cc);
        if (tail) {
            float e = 0.f;
            if (x.extra) e = x.extra[rr];
            o.s.x = (c + 0 == x.c_in && x.extra) ? e : (c + 0 == x.ones_col ? 1.f : 0.f);
            o.s.y = (c + 1 == x.c_in && x.extra) ? e : (c + 1 == x.ones_col ? 1.f : 0.f);
            o.s.z = (c + 2 == x.c_in && x.extra) ? e : (c + 2 == x.ones_col ? 1.f : 0.f);
            o.s.w = (c + 3 == x.c_in && x.extra) ? e : (c + 3 == x.ones_col ? 1.f : 0.f);
        }
    } else {
        const int cc = c < x.feat_c ? c : x.feat_c - 4;
        o.a = ldg4(x.feat + (size_t)pt * x.feat_c + cc);
        if (tail) {
            const int grp = grp_pre >= 0 ? grp_pre : x.row_grp[rr];
            const float* p = x.src_xyz + (size_t)pt * 3;
            float q0 = p[0], q1 = p[1], q2 = p[2];
            if (x.ctr_xyz) {
                const float* cp = x.ctr_xyz + (size_t)grp * 3;
                q0 = __fsub_rn(q0, cp[0]); q1 = __fsub_rn(q1, cp[1]); q2 = __fsub_rn(q2, cp[2]);
            }
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            const int t0 = c - x.feat_c;
            if (x.action) {
                const float* ap = x.action + (size_t)(grp / x.gps) * x.act_c;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ai = t0 + j - 3;
                    const int aic = ai < 0 ? 0 : (ai >= x.act_c ? x.act_c - 1 : ai);
                    const float av = ap[aic];
                    a[j] = (ai >= 0 && ai < x.act_c) ? av : 0.f;
                }
            }
            float* spv = &o.s.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = t0 + j;
                spv[j] = t == 0 ? q0 : (t == 1 ? q1 : (t == 2 ? q2 : a[j]));
            }
        }
    }
    return o;
}

// sv/tv: the layer-input BatchNorm scale/shift of this group's channels, staged in LDS
template <int XM>
__device__ __forceinline__ float4 x_finish(const XSrc& x, const XRaw& raw, bool valid, int c, const float* sv,
                                           const float* tv) {
    const int bulk = XM == 0 ? x.c_in : x.feat_c;
    const bool inside = c < bulk;
    float4 v = raw.a;
    if (XM == 0) {
        const int cc = inside ? c : x.c_in - 4;
        if (x.affine) {
            const float4 s = *reinterpret_cast<const float4*>(sv + cc), t = *reinterpret_cast<const float4*>(tv + cc);
            v.x = fmaf(v.x, s.x, t.x); v.y = fmaf(v.y, s.y, t.y); v.z = fmaf(v.z, s.z, t.z); v.w = fmaf(v.w, s.w, t.w);
        }
        if (x.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    }
    return f4sel(valid, f4sel(inside, v, raw.s), f4zero());
}

__device__ __forceinline__ void stage_vec(float* dst, const float* src, int off, int n, float fill) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = src ? src[off + i] : fill;
}

struct DzSrc {   // gad_dz_src on the device
    const float* z; int z_pitch; const float* scale; const float* shift; int relu;
    const float* P; const float* Q; const float* S; const float* row_w;
    int gmode; const float* G; int g_pitch; const int32_t* argmax; const float* dout;
    const int32_t* row_grp; int c;
    int coef;            // BatchNorm backward applies (P/Q/S given, or formed here from bw)
    int premasked;       // the ReLU mask is already in G / dout
    gad_bn_bwd bw;       // bw.dbeta != NULL: P, Q, S are formed by this launch from the layer's f64 sums
};

static DzSrc make_dzsrc(const gad_dz_src& d) {
    DzSrc s;
    s.z = d.z; s.z_pitch = d.z_pitch; s.scale = d.scale; s.shift = d.shift; s.relu = d.relu;
    s.P = d.coefP; s.Q = d.coefQ; s.S = d.coefS; s.row_w = d.row_w;
    s.gmode = d.gmode; s.G = d.G; s.g_pitch = d.g_pitch; s.argmax = d.argmax; s.dout = d.dout;
    s.row_grp = d.row_grp; s.c = d.c;
    s.premasked = d.premasked;
    s.bw.dbeta = d.bn_dbeta; s.bw.dgamma = d.bn_dgamma; s.bw.stat_stride = d.bn_stride; s.bw.count = d.bn_count;
    s.bw.mean = d.bn_mean; s.bw.istd = d.bn_istd; s.bw.gacc_gamma = d.gacc_gamma; s.bw.gacc_beta = d.gacc_beta;
    s.bw.accumulate = (d.gacc_gamma || d.gacc_beta) ? 1 : 0;
    s.coef = (d.coefP != nullptr || d.bn_dbeta != nullptr) ? 1 : 0;
    return s;
}

// P, Q, S of channel ch (identity when the layer has no BatchNorm)
// `writer`: this thread is the launch's one thread for channel ch that may add dgamma / dbeta to the gradient arena
__device__ __forceinline__ void dz_coef(const DzSrc& d, int ch, float& P, float& Q, float& S, bool writer = false) {
    if (d.bw.dbeta) gad_bn_bwd_channel(d.bw, d.scale, ch, writer, P, Q, S);
    else if (d.P) { P = d.P[ch]; Q = d.Q[ch]; S = d.S[ch]; }
    else { P = 1.f; Q = 0.f; S = 0.f; }
}
__device__ __forceinline__ bool first_workgroup() { return blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0; }

struct DzRaw { float4 z; float4 g; int4 a; };

// scalar (unaligned) evaluation of dZ[r][n..n+3], used for the tiny last layers of the heads
__device__ __forceinline__ float4 dz_scalar4(const DzSrc& d, int r, bool valid, int off, int n, int nmax) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nn = n + j;
        const bool ok = valid && nn < nmax;
        const int rr = ok ? r : 0;
        const int ch = off + (ok ? nn : 0);
        float z = 0.f;
        if (d.z) z = d.z[(size_t)rr * d.z_pitch + ch];
        float g;
        if (d.gmode == 0) {
            g = d.G[(size_t)rr * d.g_pitch + ch];
        } else {
            const int grp = d.row_grp[rr];
            g = d.argmax[(size_t)grp * d.c + ch] == r ? d.dout[(size_t)grp * d.c + ch] : 0.f;
        }
        if (d.relu && !d.premasked) {
            const float y = d.scale ? fmaf(z, d.scale[ch], d.shift[ch]) : z;
            g = y > 0.f ? g : 0.f;
        }
        if (d.P) {
            const float w = d.row_w ? d.row_w[rr] : 1.f;
            g = d.P[ch] * g - w * fmaf(d.S[ch], z, d.Q[ch]);
        }
        v[j] = ok ? g : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// raw loads of dZ's ingredients for row r, channels off+n..+3 (VEC: everything 16-byte aligned)
template <bool VEC>
__device__ __forceinline__ DzRaw dz_raw(const DzSrc& d, int r, bool valid, int off, int n, int nmax, int grp) {
    DzRaw o;
    o.z = f4zero(); o.a = make_int4(0, 0, 0, 0);
    if (!VEC) { o.g = dz_scalar4(d, r, valid, off, n, nmax); return o; }
    const int rr = valid ? r : 0;
    const int ch = off + (n < nmax ? n : 0);
    if (d.z) o.z = ldg4(d.z + (size_t)rr * d.z_pitch + ch);
    if (d.gmode == 0) {
        o.g = ldg4(d.G + (size_t)rr * d.g_pitch + ch);
    } else {
        o.a = *reinterpret_cast<const int4*>(d.argmax + (size_t)grp * d.c + ch);
        o.g = ldg4(d.dout + (size_t)grp * d.c + ch);
    }
    return o;
}

// vec: LDS copies of {scale, shift, P, Q, S} of this group's channels (VM floats each; VM = VMAX unless the kernel sizes its LDS for narrower layers)
template <bool VEC, int VM = VMAX>
__device__ __forceinline__ float4 dz_finish(const DzSrc& d, const DzRaw& raw, int r, bool valid, int n, int nmax, float w,
                                            const float* vec) {
    if (!VEC) return raw.g;
    const bool inside = n < nmax;
    const int nn = inside ? n : 0;
    float4 g = raw.g;
    const float4 z = raw.z;
    if (d.gmode != 0) {
        g.x = raw.a.x == r ? g.x : 0.f; g.y = raw.a.y == r ? g.y : 0.f;
        g.z = raw.a.z == r ? g.z : 0.f; g.w = raw.a.w == r ? g.w : 0.f;
    }
    if (d.relu && !d.premasked) {
        float4 y = z;
        if (d.scale) {
            const float4 s = *reinterpret_cast<const float4*>(vec + nn), t = *reinterpret_cast<const float4*>(vec + VM + nn);
            y.x = fmaf(z.x, s.x, t.x); y.y = fmaf(z.y, s.y, t.y); y.z = fmaf(z.z, s.z, t.z); y.w = fmaf(z.w, s.w, t.w);
        }
        g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f;
        g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
    }
    if (d.coef) {
        const float4 P = *reinterpret_cast<const float4*>(vec + 2 * VM + nn);
        const float4 Q = *reinterpret_cast<const float4*>(vec + 3 * VM + nn);
        const float4 S = *reinterpret_cast<const float4*>(vec + 4 * VM + nn);
        g.x = P.x * g.x - w * fmaf(S.x, z.x, Q.x); g.y = P.y * g.y - w * fmaf(S.y, z.y, Q.y);
        g.z = P.z * g.z - w * fmaf(S.z, z.z, Q.z); g.w = P.w * g.w - w * fmaf(S.w, z.w, Q.w);
    }
    return f4sel(valid && inside, g, f4zero());
}

template <int VM = VMAX>
__device__ __forceinline__ void stage_dz_vecs(float* vec, const DzSrc& d, int off, int n) {
    if (!d.premasked) {
        stage_vec(vec, d.scale, off, n, 1.f);
        stage_vec(vec + VM, d.shift, off, n, 0.f);
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        float P, Q, S;
        dz_coef(d, off + i, P, Q, S, first_workgroup());
        vec[2 * VM + i] = P; vec[3 * VM + i] = Q; vec[4 * VM + i] = S;
    }
}

static bool dz_vectorizable(const gad_dz_src& d, const int32_t* off, const int32_t* n_out, int ng) {
    bool ok = (d.z == nullptr || d.z_pitch % 4 == 0) && (d.gmode != 0 || d.g_pitch % 4 == 0) && (d.gmode == 0 || d.c % 4 == 0);
    for (int i = 0; i < ng; ++i) ok = ok && off[i] % 4 == 0 && n_out[i] % 4 == 0 && n_out[i] <= VMAX;
    return ok;
}

// ------------------------------------------------------------------------------------------------
// LDS tile helpers.  Tiles are k-major: T[kk][i], kk in [0,KT), i in [0,DIM).
//   transposing store (source contiguous along kk): pitch DIM+1, four ds_write_b32
//   direct store      (source contiguous along i) : pitch DIM+4, one ds_write_b128
// ------------------------------------------------------------------------------------------------
template <int DIM> struct PitchT { static constexpr int v = DIM + 1; };
template <int DIM> struct PitchD { static constexpr int v = DIM + 4; };

template <int DIM> __device__ __forceinline__ void unit_T(int u, int& i, int& kk) { i = u >> 3; kk = (u & 7) << 2; }
template <int DIM> __device__ __forceinline__ void unit_D(int u, int& kk, int& i) { kk = u / (DIM / 4); i = (u % (DIM / 4)) << 2; }

template <int DIM> __device__ __forceinline__ void store_T(float* t, int i, int kk, float4 v) {
    constexpr int P = PitchT<DIM>::v;
    t[(kk + 0) * P + i] = v.x; t[(kk + 1) * P + i] = v.y; t[(kk + 2) * P + i] = v.z; t[(kk + 3) * P + i] = v.w;
}
template <int DIM> __device__ __forceinline__ void store_D(float* t, int kk, int i, float4 v) {
    constexpr int P = PitchD<DIM>::v;
    *reinterpret_cast<float4*>(t + kk * P + i) = v;
}

// One K-tile of MFMAs.  The operand fragments are read from LDS one CHUNK (4 k-steps) ahead of the MFMAs that
// consume them: written naively (read, wait, MFMA) hipcc emits `ds_read; s_waitcnt lgkmcnt(0); v_mfma` per step and
// a lone wavefront per SIMD (the small-M layers) spends as long waiting for LDS as issuing MFMAs.
template <int TM, int TN, int PA, int PB>
__device__ __forceinline__ void mfma_ktile(const float* __restrict__ As, const float* __restrict__ Bs, int am0,
                                           int bn0, int lane, f32x16 (&acc)[TM][TN]) {
    const int l31 = lane & 31, half = lane >> 5;
    constexpr int CH = 4, NCH = KT / 2 / CH;
    const float* ap = As + half * PA + am0 + l31;
    const float* bp = Bs + half * PB + bn0 + l31;
    float a[2][CH][TM], b[2][CH][TN];
    auto fetch = [&](int c, int buf) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) a[buf][s][tm] = ap[(2 * (c * CH + s)) * PA + tm * 32];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) b[buf][s][tn] = bp[(2 * (c * CH + s)) * PB + tn * 32];
        }
    };
    fetch(0, 0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) fetch(c + 1, (c + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);       // keep the next chunk's ds_reads ABOVE this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < CH; ++s)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c & 1][s][tm], b[c & 1][s][tn], acc[tm][tn], 0, 0, 0);
    }
}

__device__ __forceinline__ int acc_row(int v, int half) { return (v & 3) + 8 * (v >> 2) + 4 * half; }

// ------------------------------------------------------------------------------------------------
// Segment max-pool folded into the epilogue of the pooled layer's GEMM (upstream _PointnetSAModuleBase.forward:
// F.max_pool2d over the nsample axis of relu(bn(conv)); reference call site core/networks.py:66-81).
// The pooled quantity is y = relu(scale * z + shift) with scale = gamma * istd: istd > 0, so the SIGN of scale is the sign
// of gamma -- known before the layer's statistics exist -- and y is monotone in z.  The epilogue therefore reduces the RAW
// output: max of sgn * z per (group, channel), sgn = +-1 from gamma; gad_pool_finalize applies the affine + ReLU to the
// winner once the statistics are in (bit-identical to pooling y: a correctly rounded fma is monotone).
// A group's rows are contiguous (CSR).  The output tile goes through LDS once so that a lane owns ONE column and walks the
// rows in order: every lane of the wavefront sees the same rows, so the segment structure (where a group ends) is
// wave-uniform -- scalar branches, group ids read with v_readlane -- and only the running maximum is per-lane work
// (compare + two selects per row).  A group that lies inside the walked row range is written with ONE plain 8-byte store
// per channel; only the groups cut by the range's ends (<= 2 per range) need a packed 64-bit atomic maximum --
// key = (order-preserving bits of the value) << 32 | ~row, so among equal values the smaller row wins (the arg-max trick
// of fps_kernel).  key 0 = "no row yet".  (First version: per-lane scan of the accumulator registers with an atomic per
// segment -- 3-4 M atomics per SA1 / SA2 launch cost 20-35 us, profiles/README.md round 3.)
// Arg-max rule vs the reference ("first maximal y"): identical unless two DIFFERENT raw values of a group round to the
// same y (then the larger raw value wins here) -- gad_pool_finalize handles y <= 0 (every row ties at 0: first row).
// ------------------------------------------------------------------------------------------------
struct PoolEpi {
    unsigned long long* key;       // (groups, C) packed keys, NULL: no pooling
    const int32_t* row_grp;        // (rows) group of every row
    const float* gamma;            // (C) BatchNorm weight of the pooled layer (its sign picks max / min)
    int C;
};

__device__ __forceinline__ unsigned pool_ord(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}

// partial (wave-uniform): the group continues outside the rows this wavefront walks
__device__ __forceinline__ void pool_put(unsigned long long* keycol, int g, int C, float v, int row, bool partial) {
    const unsigned long long k = ((unsigned long long)pool_ord(v) << 32) | (unsigned long long)(0xffffffffu - (unsigned)row);
    if (partial) atomicMax(keycol + (size_t)g * C, k);
    else keycol[(size_t)g * C] = k;
}

// running state of one lane's column: the open group (uniform), whether it began before the walked range (uniform), the
// best value so far and its row
struct PoolRun { int g; int part; float v; int row; };

// rows [i, e) of the LDS tile belong to the open group: running maximum of sgn * z, strict > (the first maximum stays),
// for NC columns per lane (zt + c * cstride).  i, e, row_base are wave-uniform: the loads of a run are independent of the
// compares and pipeline freely.
template <int NC>
__device__ __forceinline__ void pool_rows(const float* zt, int pitch, int cstride, int i, int e, int row_base, const float (&sgn)[NC],
                                          float (&best)[NC], int (&brow)[NC]) {
    int r = i;
    for (; r + 2 <= e; r += 2) {
        float z0[NC], z1[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { z0[c] = zt[r * pitch + c * cstride] * sgn[c]; z1[c] = zt[(r + 1) * pitch + c * cstride] * sgn[c]; }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            bool t = z0[c] > best[c]; best[c] = t ? z0[c] : best[c]; brow[c] = t ? row_base + r : brow[c];
            t = z1[c] > best[c]; best[c] = t ? z1[c] : best[c]; brow[c] = t ? row_base + r + 1 : brow[c];
        }
    }
    if (r < e) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float z0 = zt[r * pitch + c * cstride] * sgn[c];
            const bool t = z0 > best[c]; best[c] = t ? z0 : best[c]; brow[c] = t ? row_base + r : brow[c];
        }
    }
}

// One wavefront walks 32 consecutive rows (row_base ..) of its LDS tile, lane = column, carrying the open group across
// calls (streaming kernel: a contiguous range of slabs per wavefront).  gl: lane i < 32 holds the group of row i (-1 past
// the live rows).  A group that closes here is complete unless c.part says it began before the range.
__device__ __forceinline__ void pool_scan32(const float* zt, int pitch, int gl, int row_base, float sgn, PoolRun& c,
                                            unsigned long long* keycol, int C) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(gl, 1, 64);
    const bool st = lane == 0 ? gl != c.g : gl != prev;
    const unsigned m = (unsigned)__ballot(st);                  // bit i: row i opens a group (c.g is wave-uniform)
    int i = 0;
    while (i < 32) {                                            // wave-uniform control flow throughout
        if ((m >> i) & 1u) {
            if (c.g >= 0) pool_put(keycol, c.g, C, c.v, c.row, c.part != 0);
            c.g = __builtin_amdgcn_readlane(gl, i); c.part = 0; c.v = -INFINITY; c.row = row_base + i;
        }
        const unsigned rest = i < 31 ? m >> (i + 1) : 0u;
        const int e = rest ? i + 1 + __builtin_ctz(rest) : 32;
        if (c.g >= 0) {
            const float sg1[1] = {sgn};
            float bv[1] = {c.v};
            int br[1] = {c.row};
            pool_rows<1>(zt, pitch, 0, i, e, row_base, sg1, bv, br);
            c.v = bv[0]; c.row = br[0];
        }
        i = e;
    }
}

// A 64-row tile in LDS, lane = column (NC columns per lane, cstride apart), the tile's groups dealt to the workgroup's
// wavefronts (piece k -> wavefront k % nw): every piece is closed by the wavefront that walked it; only the pieces cut by
// the tile's first / last row are partial.
// gl: lane i holds the group of tile row i (-1 past the live rows); n_live = live rows of the tile (>= 1); g_before /
// g_after: the groups of the rows just outside the tile (-1: none) -- a piece that shares its group with them is partial.
template <int NC>
__device__ __forceinline__ void pool_tile64(const float* zt, int pitch, int cstride, int gl, int row0, int n_live,
                                            const float (&sgn)[NC], int wave, int nw, int g_before, int g_after,
                                            unsigned long long* keycol, int C) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(gl, 1, 64);
    const bool st = (lane == 0 || gl != prev) && lane < n_live;
    unsigned long long m = __ballot(st);
    int k = 0;
    while (m) {                                                 // wave-uniform
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        const int e = m ? __builtin_ctzll(m) : n_live;
        if ((k++ % nw) != wave) continue;
        const int g = __builtin_amdgcn_readlane(gl, i);
        float best[NC];
        int brow[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { best[c] = -INFINITY; brow[c] = row0 + i; }
        pool_rows<NC>(zt, pitch, cstride, i, e, row0, sgn, best, brow);
        const bool partial = (i == 0 && g == g_before) || (e == n_live && g == g_after);
#pragma unroll
        for (int c = 0; c < NC; ++c) pool_put(keycol + c * cstride, g, C, best[c], brow[c], partial);
    }
}

struct Groups {
    int n; int aoff[GAD_MAX_GROUPS]; int woff[GAD_MAX_GROUPS]; int ooff[GAD_MAX_GROUPS]; int nout[GAD_MAX_GROUPS];
};

// per-column partial sums held by lanes 0..31 of each wavefront -> one f64 atomic per column and block (STORE: the deterministic
// mode's plain store of the block's partial into its own slot, out0 / out1 = that slot)
template <int WM, int WN, int TN, bool STORE = false>
__device__ __forceinline__ void block_column_atomics(float* red, const float (&c0)[TN], const float (&c1)[TN], int lane,
                                                     int wm, int wn, int col0, int col_limit, double* out0,
                                                     double* out1) {
    constexpr int BN = WN * TN * 32;
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const float s0 = c0[tn] + __shfl_xor(c0[tn], 32, 64);
        const float s1 = c1[tn] + __shfl_xor(c1[tn], 32, 64);
        if (lane < 32) {
            const int cl = wn * TN * 32 + tn * 32 + lane;
            red[wm * BN + cl] = s0;
            red[(WM + wm) * BN + cl] = s1;
        }
    }
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < BN && col0 + tid < col_limit) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) { s0 += red[w * BN + tid]; s1 += red[(WM + w) * BN + tid]; }
        if (STORE) {
            out0[col0 + tid] = (double)s0;
            out1[col0 + tid] = (double)s1;
        } else {
            atomic_add_f64(out0 + col0 + tid, (double)s0);
            atomic_add_f64(out1 + col0 + tid, (double)s1);
        }
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- split-bf16 arithmetic (library option "mfma_split": a mask of kernel families, include/gaddpg.h GAD_SPLIT_*) ----
// An f32 value = hi + mid + lo, three bf16 terms of 8 significand bits each (the residuals are exact f32 subtractions); a product of
// two such values to 24 bits = the six term products of weight >= 2^-16, each exact in the f32 accumulator of
// v_mfma_f32_32x32x16_bf16 (16x the rate of v_mfma_f32_32x32x2_f32).  The bf16 MFMA's adder truncates toward -inf (a -1e-8
// relative bias, tools/ubench/split_bf16.hip): the products of every second block of 16 along the reduction index are
// NEGATED (one operand's sign) and summed into a second accumulator; result = plain - negated, which cancels the bias and
// leaves a smaller random error than the f32 MFMA's (profiles/r04_split_bf16_ubench.txt).  The cancellation is exact only
// where the two accumulators sit in the same binade; what is left (~2e-11 of max |z| per element) has a sign that depends on
// the output COLUMN (which half of a column's weights is larger), so a sum over the rows of one column -- BatchNorm statistics,
// dbeta -- would add it coherently.  The kernels whose outputs are summed over rows therefore also negate the A operand of
// every ODD ROW and take (negated - plain) there: the residual changes sign from row to row and averages out
// (profiles/r05_split_families.txt).
// Range: |x| must stay below 3.39e38 (bf16(x) must not round to infinity); an infinite operand gives NaN where the f32
// path gives +-inf (both non-finite).
typedef __bf16 gad_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned gad_cvt_pk_bf16(float lo, float hi) {     // {bf16(hi), bf16(lo)}, round to nearest even
    unsigned r;
    __asm__("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ void gad_split2(float a, float b, unsigned& H, unsigned& M, unsigned& L) {
    H = gad_cvt_pk_bf16(a, b);
    const f32x2 r = f32x2{a, b} - f32x2{__uint_as_float(H << 16), __uint_as_float(H & 0xffff0000u)};
    M = gad_cvt_pk_bf16(r.x, r.y);
    const f32x2 q = r - f32x2{__uint_as_float(M << 16), __uint_as_float(M & 0xffff0000u)};
    L = gad_cvt_pk_bf16(q.x, q.y);
}
__device__ __forceinline__ gad_bf16x8 gad_as_bf16x8(gad_u32x4 u) { return *reinterpret_cast<gad_bf16x8*>(&u); }

// Wide-tile kernels in split form (gemm_fwd_wide / gemm_dx_wide with SP): a 64 x 128 block tile per 4-wavefront workgroup,
// K-tile 32.  Both operand tiles live in LDS as three bf16 planes of 64-byte rows (32 reduction indices), double-buffered:
//   stage = A planes 3 x 64 rows | B planes 3 x 128 rows = 36 KB;
// a row's four 16-byte chunks are XOR-swizzled by (row >> 2) & 3, so the fragment reads -- lane (row l31, half) takes chunk
// 2 s + half of k16-step s: one ds_read_b128 = the 8 consecutive reduction indices v_mfma_f32_32x32x16_bf16 wants per lane --
// are conflict-free without padding (every 16-lane group of the instruction covers 16 rows that differ mod 16), and so are
// the staging stores (ds_write_b64 for the A side, split in registers; ds_write_b128 for the B side, copied from the
// pre-split weight mirror).  k16-step 0 of a K-tile accumulates into `acc`, step 1 -- whose mirror values are stored negated --
// into `an`.
namespace spw {
constexpr int APL = 64 * 64, BPL = 128 * 64, STAGE = 3 * (APL + BPL);       // bytes
struct BRegs { gad_u32x4 r[2][3]; };
// this thread's B chunks of K-tile kt: rows (tid >> 2) + 64 u of the block's 128 mirror rows, chunk tid & 3
__device__ __forceinline__ void load_b(BRegs& b, __amdgpu_buffer_rsrc_t rs, const int (&vb)[2], int plane_bytes, int kt) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int p = 0; p < 3; ++p) b.r[u][p] = __builtin_amdgcn_raw_buffer_load_b128(rs, vb[u], p * plane_bytes + kt * 64, 0);
}
__device__ __forceinline__ void store_b(unsigned char* stage, const BRegs& b, int tid) {
    const int row = tid >> 2;
    unsigned char* q = stage + 3 * APL + row * 64 + ((((tid & 3) ^ ((row >> 2) & 3))) << 4);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<gad_u32x4*>(q + p * BPL + u * (64 * 64)) = b.r[u][p];
}
// four consecutive reduction indices (c4 = (tid & 7) * 4 of the K-tile) of A row `row` -> the three planes (8 bytes each)
// sg: 0x80000000 for an odd row (its values enter negated, the epilogue takes negated - plain), else 0
__device__ __forceinline__ void store_a4(unsigned char* stage, int row, int tid, float4 v, unsigned sg) {
    unsigned h0, m0, l0, h1, m1, l1;
    gad_split2(__uint_as_float(__float_as_uint(v.x) ^ sg), __uint_as_float(__float_as_uint(v.y) ^ sg), h0, m0, l0);
    gad_split2(__uint_as_float(__float_as_uint(v.z) ^ sg), __uint_as_float(__float_as_uint(v.w) ^ sg), h1, m1, l1);
    unsigned char* q = stage + row * 64 + (((((tid & 7) >> 1) ^ ((row >> 2) & 3))) << 4) + ((tid & 1) << 3);
    *reinterpret_cast<uint2*>(q) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(q + APL) = make_uint2(m0, m1);
    *reinterpret_cast<uint2*>(q + 2 * APL) = make_uint2(l0, l1);
}
// MFMAs of one staged K-tile for the wavefront's 32 x 64 tile: arow / brow = byte offsets of the lane's A row and first B row
// inside the stage, fo = ((half ^ swizzle) << 4) -- the lane's chunk of k16-step 0; step 1's is fo ^ 32
__device__ __forceinline__ void ktile(const unsigned char* stage, int arow, int brow, int fo, f32x16 (&acc)[2], f32x16 (&an)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int off = fo ^ (s << 5);
        const unsigned char* ap = stage + arow + off;
        const unsigned char* bp = stage + 3 * APL + brow + off;
        const gad_u32x4 AH = *reinterpret_cast<const gad_u32x4*>(ap), AM = *reinterpret_cast<const gad_u32x4*>(ap + APL);
        const gad_u32x4 AL = *reinterpret_cast<const gad_u32x4*>(ap + 2 * APL);
        gad_u32x4 BH[2], BM[2], BL[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            BH[t] = *reinterpret_cast<const gad_u32x4*>(bp + t * (32 * 64));
            BM[t] = *reinterpret_cast<const gad_u32x4*>(bp + BPL + t * (32 * 64));
            BL[t] = *reinterpret_cast<const gad_u32x4*>(bp + 2 * BPL + t * (32 * 64));
        }
        // the six products of weight >= 2^-16, smallest first
#define GAD_SPW(A, B)                                                                                                          \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                        \
            if (s) an[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[t]), an[t], 0, 0, 0);     \
            else acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[t]), acc[t], 0, 0, 0);     \
        }
        GAD_SPW(AL, BH) GAD_SPW(AH, BL) GAD_SPW(AM, BM) GAD_SPW(AM, BH) GAD_SPW(AH, BM) GAD_SPW(AH, BH)
#undef GAD_SPW
    }
}
}  // namespace spw

// the skinny kernels (small-M layers: gemm_fwd_skinny_kernel, gemm_dx_skinny_kernel and gemm_dw_skinny_kernel, each in its pass's unit)
#define SK_NW 8          // wavefronts per workgroup (K split); 16 -> 128-VGPR budget -> spills, 2x slower
#define SK_CH 6          // 8-wide k groups per register chunk (17 x 1 = the whole K share in one round of loads: measured 2 % slower)
#define SK_SP 36         // pitch (floats) of the wavefront-private operand stage of the skinny forward kernel
#define SK_KCAP (8 * SK_NW * SK_CH * SK_MAXCH)   // most input channels of a skinny launch (per-channel affine staged in LDS)
#define SK_MAXCH 3       // chunks per wavefront: K <= 8 * SK_NW * SK_CH * SK_MAXCH = 1152
#define GAD_GX_CAP 2048           // most row tiles a tile launch spreads over workgroups (the rest by its grid-stride loop)
#define DW_STREAM_SPLITS 256

// ---- host side: the option block (gemm.hip: g_opt, gad_set_option's table) ----
struct GemmOptions {
    // family mask (GAD_SPLIT_*; 1 = all): which GEMM families multiply as split-bf16 MFMAs.  LIBRARY default 0 = v_mfma_f32_32x32x2_f32
    // throughout (round 6, ADVICE r05: a caller of the C ABI gets the reference's arithmetic unless it asks for something else); the
    // Python package opts in explicitly when it loads the library (ga-ddpg_amd/hip.py OPTION_DEFAULTS: GAD_SPLIT_ALL -- the per-family
    // float64 gates of tests/test_gpu_split_families.py, the range / specials tests and every oracle-facing gate in both modes are green
    // on MI355X), GAD_OPT_mfma_split=0 keeps the f32 MFMA.  Precondition of the split form: finite operands below 3.39e38 in magnitude
    // (bf16(x) must not round to infinity; an infinite operand gives NaN where the f32 path gives +-inf).
    int mfma_split = 0;
    int deterministic = 0;        // the generic tile kernels only, ordered partial sums (gemm.hip, "deterministic mode")
    int fwd_wide = 1, dx_wide = 1, dw_wide = 1;    // the wide-tile routes (2: not for the gathered first layers)
    int bwd_fused = 1;            // gad_gemm_bwd: the fused SA1 streaming backward
    int fwd_bn_prologue = 1;      // 0: routes with a BatchNorm-finalising prologue launch gad_bn_finalize instead (A/B)
    int bwd_wide = 0;             // fused wide backward: 0 off (default: slower in the step), 1 SA2 and SA3 shapes, 2 only layers with >= 16384 rows (SA2)
    int bwd_wide_slab = 4;        // most partial-dW elements (millions) a fused launch may write: bounds its workgroups per k block
    int dw_wide_wgs = 256;        // workgroups a wide-tile dW launch aims for (its partial slab = this x 128 x 128 floats)
    int skinny_nw = SK_NW;        // wavefronts per skinny workgroup: 8, or 4 (A/B: a quarter of a CU's registers and < 60 KB of LDS, so a workgroup fits beside the side lanes' wide kernels)
    int fwd_skinny = 1, dx_skinny = 1, dx_stream = 1, dw_skinny = 1, dw_stream = 1, fwd_stream = 1;   // the skinny and streaming routes
    int bwd_stream_wgs = DW_STREAM_SPLITS;   // persistent workgroups (= partial dW blocks) of the fused SA1 backward: A/B, <= DW_STREAM_SPLITS
    int fwd_stream_wgs = 256;     // persistent workgroups of the streaming forward's layers 2 / 3 (A/B: fewer leave CUs to the sibling pass's small launches)
    int fwd_stream_l1_wgs = 256;  // persistent workgroups of the streaming forward's gathered first layer (A/B: 512 = two per CU)
};
extern GemmOptions g_opt;
bool split_on(int family);      // the family multiplies as split-bf16 MFMAs (never in deterministic mode)

// the skinny launch of every pass: 4 wavefronts per workgroup under option "skinny_nw" = 4, else SK_NW
#define GAD_LAUNCH_SKINNY(kernel, grid, st, ...)                                                                               \
    do {                                                                                                                       \
        if (g_opt.skinny_nw == 4) hipLaunchKernelGGL(kernel<4>, grid, dim3(64 * 4), 0, st, __VA_ARGS__);                       \
        else hipLaunchKernelGGL(kernel<SK_NW>, grid, dim3(64 * SK_NW), 0, st, __VA_ARGS__);                                    \
    } while (0)

static Groups make_groups(int n, const int32_t* a, const int32_t* w, const int32_t* o, const int32_t* no) {
    Groups g;
    g.n = n;
    for (int i = 0; i < GAD_MAX_GROUPS; ++i) {
        g.aoff[i] = (i < n && a) ? a[i] : 0; g.woff[i] = (i < n && w) ? w[i] : 0;
        g.ooff[i] = (i < n && o) ? o[i] : 0; g.nout[i] = i < n ? no[i] : 0;
    }
    return g;
}

static int max_nout(const Groups& g) { int m = 0; for (int i = 0; i < g.n; ++i) m = g.nout[i] > m ? g.nout[i] : m; return m; }

struct DxEpi {
    int mode; float* gout; int gout_pitch; int k_valid;
    const float* zprev; int zprev_pitch; const float* ps; const float* pt; const float* pm; const float* pi;
    double* dbeta; double* dgamma; int stat_stride; int store_masked;
    float* dfeat; int feat_c; const int32_t* row_pt; const int32_t* row_grp; double* daction; int act_c; int gps;
};

static DxEpi make_dxepi(const gad_gemm_dx_args& a) {
    DxEpi e;
    e.mode = a.epilogue; e.gout = a.gout; e.gout_pitch = a.gout_pitch; e.k_valid = a.k_valid;
    e.zprev = a.zprev; e.zprev_pitch = a.zprev_pitch; e.ps = a.prev_scale; e.pt = a.prev_shift;
    e.pm = a.prev_mean; e.pi = a.prev_istd; e.dbeta = a.prev_dbeta; e.dgamma = a.prev_dgamma;
    e.stat_stride = a.stat_stride;
    e.store_masked = (a.store_masked && a.prev_dbeta) ? 1 : 0;
    e.dfeat = a.dfeat; e.feat_c = a.feat_c; e.row_pt = a.row_pt; e.row_grp = a.row_grp;
    e.daction = a.daction; e.act_c = a.act_c; e.gps = a.grp_per_sample > 0 ? a.grp_per_sample : 1;
    return e;
}

// ---- host functions that cross the units ----
// gemm.hip
int check_input(const gad_gemm_fwd_args& a, const char* who);
int coef_fallback(gad_dz_src& dz, void* stream);
bool fits_i32_bytes(long long rows, int pitch_a, int pitch_b, int pitch_c, int pitch_d);
double* det_stat_slots(int gx, int ncol, void* stream);
int det_stat_reduce(const double* slots, int gx, int ncol, double* sum, double* sq, void* stream);
// gemm_fwd.hip: the streaming forward route's predicate (check_input: mode 2 exists in that form only)
bool fwd_streamable(const gad_gemm_fwd_args& a);
// gemm_bwd.hip, with the streaming backward family: the SA1 streaming dX route's predicate and its launch, gad_gemm_dx's first route
bool dx_streamable(const gad_gemm_dx_args& a, bool vec);
int dx_stream_launch(const gad_gemm_dx_args* a, const DzSrc& d, const DxEpi& e, unsigned long long* ts, void* stream);
// gemm_dw.hip: the streaming dW route's predicate (gad_gemm_bwd fuses what it and dx_streamable both cover), and dw_reduce_kernel
// over `splits` partial blocks of nmax x Kp floats per group, summed into gacc
bool dw_streamable(const gad_gemm_dw_args& a, int k_used);
int dw_reduce_launch(const float* partial, const Groups& gr, int nmax, const int32_t* n_rows_dev, int rows, int splits, int Kp,
                     int k_used, double* gacc, int all_active, hipStream_t st);
