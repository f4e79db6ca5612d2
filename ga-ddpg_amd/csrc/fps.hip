// PointNet++ geometry operators for gfx950: furthest point sampling, ball query, grouping (+grad), gather (+grad), feature
// propagation, and the compaction of ball-query output into de-duplicated neighbourhood rows.
// Replaces the CUDA kernels of the reference's external `pointnet2_ops._ext` (sampling_gpu.cu, ball_query_gpu.cu,
// group_points_gpu.cu, interpolate_gpu.cu; reached from reference core/networks.py:66-81).
// Design (MI355X-first, not a translation): wave64 ballot/prefix-popcount compaction for the ball query (one wavefront per
// centroid instead of one thread), register-resident clouds with a shuffle arg-max for FPS (one workgroup per cloud, no global
// scratch), 16-byte coalesced streams for the materialising group kernels.
//
// Map of the units (a kernel template is defined and instantiated in exactly one unit):
//   fps.hip          this file: gad_furthest_point_sampling (fps_kernel<points per lane, wavefronts>) and gad_fps_tiled for any size
//   ball_query.hip   gad_ball_query (scan, LDS-tiled, cell list), gad_ball_query_grid, gad_query_and_group: one route decision
//   group.hip        gad_group_points / gad_gather_points and their gradients, gad_prep_points, the row builders of the fused path
//   interpolate.hip  gad_three_nn, gad_three_nn_grid, gad_three_interpolate and its gradients (the deterministic one through
//                    group.hip's group_points_grad_weighted_launch)
//   point_grid.hip   the uniform grid in global memory behind the two *_grid operators (point_grid.hpp)
//   library.hip      no kernel: error string, timing slot, hints, ABI version, and the option block of these units (common.hpp)
#include "common.hpp"
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// furthest point sampling
// ------------------------------------------------------------------------------------------------
// Arg-max candidates are packed as (float bits of the distance) << 32 | ~key: distances are >= +0, so their bit patterns
// order like the values, and among equal distances the SMALLER key must win (see the tie rule below); 0 = "no candidate".
// pack(a) > pack(b)  <=>  a.v > b.v || (a.v == b.v && a.key < b.key), the upstream comparison.
__device__ __forceinline__ unsigned long long fps_pack(float v, unsigned key) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(unsigned)(~key);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long fps_dpp_max(unsigned long long v) {      // lanes without a source keep v
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)v, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    const unsigned long long o = ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
    return o > v ? o : v;
}
// wavefront maximum (uniform result): DPP row shifts / row broadcasts instead of six ds_bpermute round trips
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v) {
    v = fps_dpp_max<0x111, 0xf>(v); v = fps_dpp_max<0x112, 0xf>(v); v = fps_dpp_max<0x114, 0xf>(v); v = fps_dpp_max<0x118, 0xf>(v);
    v = fps_dpp_max<0x142, 0xa>(v);                                // row_bcast:15 -> rows 1, 3
    v = fps_dpp_max<0x143, 0xc>(v);                                // row_bcast:31 -> rows 2, 3: lane 63 holds the maximum
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// wavefront maximum of a float / minimum of an unsigned (uniform results), same DPP ladder
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float fps_dpp_fmax(float v) {
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
    return o > v ? o : v;
}
__device__ __forceinline__ float fps_wave_fmax(float v) {
    v = fps_dpp_fmax<0x111, 0xf>(v); v = fps_dpp_fmax<0x112, 0xf>(v); v = fps_dpp_fmax<0x114, 0xf>(v); v = fps_dpp_fmax<0x118, 0xf>(v);
    v = fps_dpp_fmax<0x142, 0xa>(v);
    v = fps_dpp_fmax<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// the same ladder as ONE instruction per step (v_max_f32 with a DPP source; a lane without a source is not written and keeps
// its own value).  hipcc turns the select form above into v_mov / v_mov_dpp / v_cmp / v_cndmask + hazard s_nops: 4x the issue
// slots on the one dependent chain every arg-max round waits for.  (s_nop 1: VALU write -> DPP read of the same register.)
__device__ __forceinline__ float fps_wave_fmax_asm(float v) {
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
                 "s_nop 1" : "+v"(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// v_min_f32 / v_max3_f32 as they are, no canonicalising v_max x, x in front.  A distance CAN be NaN (a NaN coordinate, inf - inf;
// gaddpg.h defines the picks for such clouds) and the instructions are still right: the NaN is the result of an arithmetic
// instruction, hence quiet, and v_min_f32 of a quiet NaN and a number returns the number -- upstream's `d < temp ? d : temp`, which
// keeps temp.  temp therefore never becomes NaN (it starts as the -1 sentinel or 1e10 and only ever takes a smaller non-NaN
// distance; +inf loses against 1e10 too), so v_max3_f32 and the `tm == bd` / `bd == dmax` compares never see one.
__device__ __forceinline__ float fps_vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float fps_vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float fps_settle(float v) {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned fps_dpp_umin(unsigned v) {
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned fps_wave_umin(unsigned v) {
    v = fps_dpp_umin<0x111, 0xf>(v); v = fps_dpp_umin<0x112, 0xf>(v); v = fps_dpp_umin<0x114, 0xf>(v); v = fps_dpp_umin<0x118, 0xf>(v);
    v = fps_dpp_umin<0x142, 0xa>(v);
    v = fps_dpp_umin<0x143, 0xc>(v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

#ifdef GAD_FPS_PHASES
// diagnostic build (tools/ubench_fps.py --phases): cycles wavefront 0 of workgroup 0 spends in each part of an arg-max round
__device__ unsigned long long gad_fps_phase[8];
#define FPS_T(i) do { const unsigned long long t1_ = __builtin_readcyclecounter(); if (blockIdx.x == 0 && threadIdx.x == 0) gad_fps_phase[i] += t1_ - t0_; t0_ = __builtin_readcyclecounter(); } while (0)
extern "C" int gad_fps_phase_read(unsigned long long* out8, int reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (out8) hipMemcpyFromSymbol(out8, HIP_SYMBOL(gad_fps_phase), sizeof(z));
    if (reset) hipMemcpyToSymbol(HIP_SYMBOL(gad_fps_phase), z, sizeof(z));
    return 0;
}
#else
#define FPS_T(i) do { } while (0)
#endif
// One workgroup (WAVES wavefronts) per cloud; thread t keeps points k = s*T + t (s < NPL) in
// registers.  The cloud is also staged in LDS so the coordinates of the last pick are a broadcast
// LDS read.  Tie rule == the upstream block reduction: "thread" t = k mod tie_bs keeps its lowest k
// (strict >), and the pairwise tree `v2 > v1 ? i2 : i1` over strides bs/2..1 lets the candidate with
// the smallest BIT-REVERSED thread id win among equal values (slot t beats slot t+s at every level).
// (the library is built without packed-f32 instructions -- csrc/Makefile; this kernel opts back in: its packed
// operands are the points' long-lived register pairs and SCALAR pick coordinates, never a pair fresh from an LDS read, and the
// distance update is half of its round)
template <int NPL, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((target("packed-fp32-ops"))) void fps_kernel(const float* __restrict__ xyz, int N, int M,
                                                          int tie_bits, int32_t* __restrict__ idx,
                                                          float* __restrict__ new_xyz) {
    constexpr int T = 64 * WAVES;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sp = lds;                                   // N*3 coordinates
    unsigned long long* red = reinterpret_cast<unsigned long long*>(lds + ((N * 3 + 3) & ~3));   // 2 x WAVES packed maxima
    int* pk = reinterpret_cast<int*>(lds + ((N * 3 + 3) & ~3) + 64);                             // the M picks (written out at the end)
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = xyz + (size_t)b * N * 3;
    for (int i = tid; i < N * 3; i += T) sp[i] = p[i];
    __syncthreads();
    int old = 0;
    if (tid == 0 && M > 0) pk[0] = 0;
    auto key_of = [&](int k) {
        const unsigned t = (unsigned)k & ((1u << tie_bits) - 1u);              // k mod tie_bs
        const unsigned rev = tie_bits ? (__brev(t) >> (32 - tie_bits)) : 0u;
        return (rev << 16) | (unsigned)k;
    };
#ifdef GAD_FPS_PHASES
    unsigned long long t0_ = __builtin_readcyclecounter();
#endif
    auto publish = [&](int j, unsigned long long best) {           // cross-wavefront maximum, the pick, its output
        if (WAVES > 1) {                                           // one barrier per pick: the exchange buffer alternates
            unsigned long long* r = red + (j & 1) * WAVES;
            if ((tid & 63) == 0) r[tid >> 6] = best;
            __syncthreads();
            FPS_T(4);
            best = r[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) best = r[w] > best ? r[w] : best;
        }
        const unsigned bkey = best ? ~(unsigned)best : 0u;         // no candidate at all (every point skipped): index 0
        const int pick = (int)(bkey & 0xFFFFu);
        // the pick goes to LDS, the outputs are written once all M are known: a global store (and the LDS read of the pick's
        // coordinates for it) in here sat on wavefront 0's path to the next barrier -- 150 of a round's ~1300 cycles
        if (tid == 0) pk[j] = pick;
        FPS_T(5);
        return pick;
    };
    if constexpr (NPL % 2 == 0) {
        // ---- fast path (round 5).  The thread's points live as packed PAIRS (v_pk_*_f32 operands as they are: the first version
        // re-packed scalar arrays every round and the 16-point instantiation ran with 248 + 256 registers and 772 bytes of
        // scratch per lane), a skipped / absent point is a point whose temp is -1 (never updated -- min(d, -1) = -1 -- and never
        // a candidate), and the arg-max needs no 64-bit compare: the thread visits its points in ASCENDING KEY ORDER with a strict
        // '>' on the float distance (the first maximum = the smallest key stays), the wavefront takes the float maximum with a
        // DPP ladder and then asks which lanes hold it: one lane -> its key by v_readlane, several (exact ties) -> the smallest
        // key among them.  Key order inside a thread: key = (bit-reversed (k mod tie_bs) << 16) | k, k = s * T + tid: for
        // tie_bs <= T the keys ascend with s; for tie_bs = 2 T (T = 256, N >= 512) the even s come first.
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        constexpr int H = NPL / 2;
        f32x2_t qx[H], qy[H], qz[H], tm[H];
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = (2 * h + u) * T + tid;
                const int kk = k < N ? k : N - 1;
                // (through a v_mov each: the packed instructions below must not be the first readers of registers an LDS read has just
                // filled -- DESIGN.md section 5; a scalar instruction in that position is safe)
                const float x = fps_settle(sp[kk * 3 + 0]), y = fps_settle(sp[kk * 3 + 1]), z = fps_settle(sp[kk * 3 + 2]);
                // upstream: `if (mag <= 1e-3) continue;` compares the FLOAT mag with the DOUBLE literal: the float nearest to 0.001
                // (0x3A83126F = 0.00100000005) is > 0.001 and therefore NOT skipped -- in float terms "skip iff mag < 1e-3f"
                const bool skip = k >= N || gad_sqnorm(x, y, z) < 1e-3f;
                qx[h][u] = x; qy[h][u] = y; qz[h][u] = z;
                tm[h][u] = skip ? -1.f : 1e10f;
            }
        const int ratio = (1 << tie_bits) / T;              // (tie_bs <= 512: at most 8 for one wavefront per cloud)
        for (int j = 1; j < M; ++j) {
            const float* po = sp + ((old << 1) + old);
            // the pick's coordinates as wave-uniform SCALARS (v_readfirstlane of the broadcast LDS read)
            const float x1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(po[0])));
            const float y1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(po[1])));
            const float z1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(po[2])));
            {
                // two points per instruction, each operation individually rounded like the scalar gad_sqdist (contraction off: the
                // indices must stay bit-identical to upstream's)
#pragma clang fp contract(off)
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const f32x2_t dx = qx[h] - x1, dy = qy[h] - y1, dz = qz[h] - z1;
                    const f32x2_t xx = dx * dx, yy = dy * dy, zz = dz * dz;
                    const f32x2_t dd = (xx + yy) + zz;
                    tm[h][0] = fps_vmin(dd[0], tm[h][0]);
                    tm[h][1] = fps_vmin(dd[1], tm[h][1]);
                }
            }
            FPS_T(0);
            // the thread's maximum by a v_max3 tree -- the wavefront maximum below starts from it at once -- and, in its shadow,
            // WHICH of the thread's points holds it: the first in ascending key order (upstream's strict '>' keeps the smallest key
            // among equal distances), found by walking the points in DESCENDING key order with independent compares
            float bd;
            if constexpr (NPL == 2) {
                bd = fps_vmax3(tm[0][0], tm[0][1], -1.f);
            } else {
                float lv[NPL / 2];
#pragma unroll
                for (int h = 0; h < H; h += 1) lv[h] = h == 0 ? fps_vmax3(tm[0][0], tm[0][1], -1.f) : fps_vmax3(tm[h][0], tm[h][1], lv[h - 1]);
                bd = lv[H - 1];
            }
            const float dmax = fps_wave_fmax_asm(bd);
            FPS_T(2);
            int bs = 0;
            // key order: R = tie_bs / T (upstream's block vs this workgroup); key's leading part is the bit-reversed (s mod R),
            // then k: so s = m, m + R, m + 2 R, ... for m in bit-reversed counting order -- walked backwards here
            auto visit = [&](auto rc) {
                constexpr int R = decltype(rc)::value;
                constexpr int LR = R == 1 ? 0 : (R == 2 ? 1 : (R == 4 ? 2 : 3));
#pragma unroll
                for (int c = R - 1; c >= 0; --c) {
                    const int m = LR == 0 ? 0 : (int)(__builtin_bitreverse32((unsigned)c) >> (32 - (LR ? LR : 1)));
                    if (m < NPL) {
#pragma unroll
                        for (int q = (NPL - 1 - m) / R; q >= 0; --q) { const int s = m + q * R; bs = tm[s >> 1][s & 1] == bd ? s : bs; }
                    }
                }
            };
            if (ratio <= 1) visit(std::integral_constant<int, 1>());
            else if (ratio == 2) visit(std::integral_constant<int, 2>());
            else if (ratio == 4) visit(std::integral_constant<int, 4>());
            else visit(std::integral_constant<int, 8>());
            FPS_T(1);
            unsigned long long best = 0ull;
            if (dmax >= 0.f) {
                const unsigned bk = key_of(bs * T + tid);
                const unsigned long long tied = __ballot(bd == dmax);
                unsigned kb;
                if (__builtin_popcountll(tied) == 1) kb = (unsigned)__builtin_amdgcn_readlane((int)bk, __builtin_ctzll(tied));
                else kb = fps_wave_umin(bd == dmax ? bk : 0xffffffffu);
                best = fps_pack(dmax, kb);
            }
            FPS_T(3);
            old = publish(j, best);
        }
    } else {
        float px[NPL], py[NPL], pz[NPL], tmp[NPL];
        unsigned key[NPL];
        unsigned valid = 0;
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int k = s * T + tid;
            px[s] = py[s] = pz[s] = 0.f;
            tmp[s] = 1e10f;
            key[s] = 0;
            if (k < N) {
                px[s] = sp[k * 3 + 0];
                py[s] = sp[k * 3 + 1];
                pz[s] = sp[k * 3 + 2];
                const float mag = gad_sqnorm(px[s], py[s], pz[s]);
                if (!(mag < 1e-3f)) valid |= 1u << s;              // (the float-vs-double-literal compare: see the fast path)
                key[s] = key_of(k);
            }
        }
        for (int j = 1; j < M; ++j) {
            const float x1 = sp[old * 3 + 0], y1 = sp[old * 3 + 1], z1 = sp[old * 3 + 2];
            unsigned long long best = 0ull;
#pragma unroll
            for (int s = 0; s < NPL; ++s) {
                if (valid & (1u << s)) {
                    const float d = gad_sqdist(px[s], py[s], pz[s], x1, y1, z1);
                    const float d2 = d < tmp[s] ? d : tmp[s];
                    tmp[s] = d2;
                    const unsigned long long c = fps_pack(d2, key[s]);
                    best = c > best ? c : best;
                }
            }
            old = publish(j, fps_wave_max(best));
        }
    }
    __syncthreads();
    for (int j = tid; j < M; j += T) {
        const int pick = pk[j];
        idx[(size_t)b * M + j] = pick;
        if (new_xyz) {
            float* o = new_xyz + ((size_t)b * M + j) * 3;
            o[0] = sp[pick * 3 + 0]; o[1] = sp[pick * 3 + 1]; o[2] = sp[pick * 3 + 2];
        }
    }
}

static int fps_tie_bits(int n) {  // log2 of upstream opt_n_threads(n) = pow2 <= min(n, 512)
    int bits = 0;
    while ((2 << bits) <= n && (2 << bits) <= 512) ++bits;
    return bits;
}

extern "C" int gad_furthest_point_sampling(const float* xyz, int B, int N, int M, int32_t* idx,
                                           float* new_xyz, void* stream) {
    GAD_REQUIRE(xyz && idx, GAD_ERR_NULL, "fps: null pointer");
    GAD_REQUIRE(B >= 0 && N >= 1 && M >= 0 && N <= 16384 && N <= 65535, GAD_ERR_SHAPE, "fps: unsupported shape B=%d N=%d M=%d", B, N, M);
    // (upstream accepts npoint > N: once every distance is 0 its tie rule picks the index.  This kernel keeps the M picks next to
    // the cloud in LDS and refuses the shape; gad_fps_tiled below takes it)
    GAD_REQUIRE(M <= N, GAD_ERR_SHAPE, "fps: M=%d picks from N=%d points", M, N);
    if (B == 0 || M == 0) return GAD_OK;
    hipStream_t st = (hipStream_t)stream;
    const int tie = fps_tie_bits(N);
    const size_t lds = (size_t)(((N * 3 + 3) & ~3) + 64 + M) * sizeof(float);      // coordinates, exchange slots, picks
    // one workgroup holds its whole cloud in LDS: 160 KB per CU bounds N (N = M: 10 220 points); beyond 64 KB the kernel's dynamic
    // LDS limit has to be raised first (such a launch used to fail at hipGetLastError)
    GAD_REQUIRE(lds <= 160 * 1024, GAD_ERR_SHAPE, "fps: N=%d, M=%d need %zu bytes of LDS per cloud (the CU has 163840)", N, M, lds);
#define FPS_LAUNCH(PPL, WV)                                                                                                   \
    do {                                                                                                                      \
        auto kern = fps_kernel<PPL, WV>;                                                                                      \
        if (lds > 64 * 1024 &&                                                                                                \
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { \
            gad_set_error("fps: cannot raise the dynamic LDS limit to %zu bytes", lds);                                       \
            return GAD_ERR_LAUNCH;                                                                                            \
        }                                                                                                                     \
        hipLaunchKernelGGL(kern, dim3(B), dim3(64 * WV), lds, st, xyz, N, M, tie, idx, new_xyz);                              \
    } while (0)
    if (N <= 64) {
        FPS_LAUNCH(1, 1);
    } else if (N <= 1024) {
        if (g_geo_opt.fps_cfg == 3) FPS_LAUNCH(16, 1);
        else if (g_geo_opt.fps_cfg == 4) FPS_LAUNCH(8, 2);
        else FPS_LAUNCH(4, 4);
    } else if (N <= 4096) {
        if (g_geo_opt.fps_cfg == 3) FPS_LAUNCH(64, 1);
        else if (g_geo_opt.fps_cfg == 4) FPS_LAUNCH(32, 2);
        else if (g_geo_opt.fps_cfg == 1) FPS_LAUNCH(8, 8);
        else if (g_geo_opt.fps_cfg == 2) FPS_LAUNCH(4, 16);
        else FPS_LAUNCH(16, 4);
    } else {
        FPS_LAUNCH(16, 16);
    }
#undef FPS_LAUNCH
    GAD_CHECK_LAUNCH("fps");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// furthest point sampling of clouds that do not fit one workgroup (raw depth clouds: 1e5 .. 3e5 points; npoint > N)
// ------------------------------------------------------------------------------------------------
// A cloud is cut into `groups` contiguous slices, one workgroup each; the running minimum distances (upstream's `temp` tensor)
// live in the caller's workspace, -1 marking a point the skip rule excludes (min(d, -1) stays -1, and -1 is never a candidate).
// ONE LAUNCH PER ROUND: round j reads the pick of round j - 1 from that round's slot, updates its slice, reduces it to one packed
// (distance bits, inverted key) maximum and folds it into slot j with a 64-bit device-scope atomic max.  The stream orders the
// rounds; no workgroup ever waits for another inside a launch (no grid barrier, no spinning: a grid-wide sync measured 2-3x a
// dependent launch on this part, profiles/HISTORY_design_notes_r01_r04.md).  A slot is written by round j only and read by the
// launches after it, so the maximum of unsigned integers is the same whatever the arrival order: the picks are deterministic.
// The key is (bit-reversed (k mod tie_bs) << 22) | k -- 9 + 22 bits, hence the cap on N; slot value 0 = "no candidate" = index 0.
#define FPS_TILED_MAX_N (1 << 22)
#define FPS_TILED_T 256
#define FPS_TILED_SLICE 1024                       // points per workgroup when the caller passes groups = 0 (profiles/fps_tiled.txt)

__device__ __forceinline__ int fps_tiled_pick(unsigned long long best) {
    return best ? (int)(~(unsigned)best & (unsigned)(FPS_TILED_MAX_N - 1)) : 0;
}

__global__ __launch_bounds__(FPS_TILED_T) void fps_tiled_init_kernel(const float* __restrict__ xyz, long long n_points,
                                                                     float* __restrict__ temp, unsigned long long* __restrict__ slots,
                                                                     long long n_slots) {
    const long long stride = (long long)gridDim.x * FPS_TILED_T;
    for (long long i = (long long)blockIdx.x * FPS_TILED_T + threadIdx.x; i < n_points; i += stride) {
        const float* q = xyz + i * 3;
        temp[i] = gad_sqnorm(q[0], q[1], q[2]) < 1e-3f ? -1.f : 1e10f;           // (the float form of upstream's compare: see fps_kernel)
    }
    for (long long i = (long long)blockIdx.x * FPS_TILED_T + threadIdx.x; i < n_slots; i += stride) slots[i] = 0ull;
}

__global__ __launch_bounds__(FPS_TILED_T) void fps_tiled_round_kernel(const float* __restrict__ xyz, int N, int M, int j, int groups,
                                                                      int slice, int tie_bits, float* __restrict__ temp,
                                                                      unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long red[FPS_TILED_T / 64];
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups, tid = threadIdx.x;
    const int k0 = g * slice, k1 = min(N, k0 + slice);
    if (k0 >= k1) return;                                            // (workgroup-uniform: trailing slices of an uneven cut are empty)
    const float* p = xyz + (size_t)b * N * 3;
    float* t = temp + (size_t)b * N;
    unsigned long long* s = slots + (size_t)b * M;
    const int old = fps_tiled_pick(s[j - 1]);                        // (slot 0 stays 0: the first pick is index 0)
    const float x1 = p[old * 3 + 0], y1 = p[old * 3 + 1], z1 = p[old * 3 + 2];
    const unsigned tie_mask = (1u << tie_bits) - 1u;
    unsigned long long best = 0ull;
#pragma unroll 4
    for (int k = k0 + tid; k < k1; k += FPS_TILED_T) {
        float tv = t[k];
        if (tv >= 0.f) {
            const float d = gad_sqdist(p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2], x1, y1, z1);
            if (d < tv) {
                tv = d;
                t[k] = d;
            }
            const unsigned rev = tie_bits ? (__brev((unsigned)k & tie_mask) >> (32 - tie_bits)) : 0u;
            const unsigned long long c = fps_pack(tv, (rev << 22) | (unsigned)k);
            best = c > best ? c : best;
        }
    }
    best = fps_wave_max(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < FPS_TILED_T / 64; ++w) best = red[w] > best ? red[w] : best;
        if (best) __hip_atomic_fetch_max(s + j, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(FPS_TILED_T) void fps_tiled_write_kernel(const float* __restrict__ xyz, int N, int M, long long n_slots,
                                                                      const unsigned long long* __restrict__ slots,
                                                                      int32_t* __restrict__ idx, float* __restrict__ new_xyz) {
    const long long stride = (long long)gridDim.x * FPS_TILED_T;
    for (long long i = (long long)blockIdx.x * FPS_TILED_T + threadIdx.x; i < n_slots; i += stride) {
        const int pick = fps_tiled_pick(slots[i]);
        idx[i] = pick;
        if (new_xyz) {
            const float* q = xyz + ((i / M) * N + pick) * 3;
            float* o = new_xyz + i * 3;
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        }
    }
}

// argument checks shared by the two entry points; *groups receives the workgroups per cloud in force
static int fps_tiled_check(const char* who, int B, int N, int M, int* groups) {
    GAD_REQUIRE(B >= 0 && N >= 1 && M >= 0, GAD_ERR_SHAPE, "%s: unsupported shape B=%d N=%d M=%d", who, B, N, M);
    GAD_REQUIRE(N <= FPS_TILED_MAX_N, GAD_ERR_SHAPE, "%s: N=%d is over the cap of %d points (22 index bits of the arg-max key)", who, N,
                FPS_TILED_MAX_N);
    GAD_REQUIRE(*groups >= 0 && *groups <= N, GAD_ERR_SHAPE, "%s: groups=%d outside [0, N=%d]", who, *groups, N);
    if (*groups == 0) *groups = gad_cdiv(N, FPS_TILED_SLICE);
    // (hipLaunchKernelGGL takes the grid in threads: workgroups x 256 has to stay below 2^32)
    GAD_REQUIRE((long long)B * *groups < (1ll << 23), GAD_ERR_SHAPE, "%s: a grid of B * groups = %d * %d workgroups overflows", who, B,
                *groups);
    return GAD_OK;
}

static long long fps_tiled_temp_bytes(int B, int N) { return ((long long)B * N * 4 + 255) & ~255ll; }

extern "C" long long gad_fps_tiled_workspace_bytes(int B, int N, int M, int groups) {
    const int rc = fps_tiled_check("fps_tiled_workspace_bytes", B, N, M, &groups);
    if (rc != GAD_OK) return rc;
    return fps_tiled_temp_bytes(B, N) + (long long)B * M * 8;       // temp (B,N) f32, then one 64-bit slot per cloud and round
}

extern "C" int gad_fps_tiled(const float* xyz, int B, int N, int M, int groups, int32_t* idx, float* new_xyz, void* workspace,
                             void* stream) {
    GAD_REQUIRE(xyz && idx, GAD_ERR_NULL, "fps_tiled: null pointer (xyz / idx)");
    const int rc = fps_tiled_check("fps_tiled", B, N, M, &groups);
    if (rc != GAD_OK) return rc;
    if (B == 0 || M == 0) return GAD_OK;
    GAD_REQUIRE(workspace, GAD_ERR_NULL, "fps_tiled: null pointer (workspace)");
    GAD_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, GAD_ERR_SHAPE, "fps_tiled: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* temp = static_cast<float*>(workspace);
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + fps_tiled_temp_bytes(B, N));
    const long long n_points = (long long)B * N, n_slots = (long long)B * M;
    const int slice = gad_cdiv(N, groups), tie = fps_tie_bits(N);
    const long long n_max = n_points > n_slots ? n_points : n_slots;
    const int init_grid = (int)(gad_cdiv(n_max, FPS_TILED_T) < 4096 ? gad_cdiv(n_max, FPS_TILED_T) : 4096);
    hipLaunchKernelGGL(fps_tiled_init_kernel, dim3(init_grid), dim3(FPS_TILED_T), 0, st, xyz, n_points, temp, slots, n_slots);
    for (int j = 1; j < M; ++j)
        hipLaunchKernelGGL(fps_tiled_round_kernel, dim3(B * groups), dim3(FPS_TILED_T), 0, st, xyz, N, M, j, groups, slice, tie, temp,
                           slots);
    const int out_grid = (int)(gad_cdiv(n_slots, FPS_TILED_T) < 4096 ? gad_cdiv(n_slots, FPS_TILED_T) : 4096);
    hipLaunchKernelGGL(fps_tiled_write_kernel, dim3(out_grid), dim3(FPS_TILED_T), 0, st, xyz, N, M, n_slots, slots, idx, new_xyz);
    GAD_CHECK_LAUNCH("fps_tiled");
    return GAD_OK;
}
