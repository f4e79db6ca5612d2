// Forward pass of the layer-GEMM family (overview and map of the units: gemm.hip): the tile, wide, streaming and skinny kernels,
// their route predicates and gad_gemm_fwd.
#include "gemm_common.hpp"

// ------------------------------------------------------------------------------------------------
// forward:  zout[r][n] = sum_k X[r][k] * W[n][k]      (+ weighted BatchNorm statistics)
// ------------------------------------------------------------------------------------------------
// DET (deterministic mode): stat_sum / stat_sq are slot planes of stat_stride doubles per block; block x stores its partial in row x
template <int WM, int WN, int TM, int TN, int XM, bool POOL, bool DET = false>
__global__ __launch_bounds__(256) void gemm_fwd_kernel(XSrc x, Groups gr, const int32_t* __restrict__ n_rows_dev,
                                                        int n_rows_static, const float* __restrict__ row_w,
                                                        const float* __restrict__ W, int Kp,
                                                        float* __restrict__ zout, int zout_pitch,
                                                        double* __restrict__ stat_sum,
                                                        double* __restrict__ stat_sq, int stat_stride, PoolEpi pe,
                                                        unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int PA = PitchT<BM>::v, PB = PitchT<BN>::v;
    constexpr int UA = BM * 8 / 256, UB = BN * 8 / 256;
    constexpr int TILE = KT * PA + KT * PB;
    constexpr int SM = ((TILE + 3) & ~3) + 2 * BM + 2 * VMAX;
    static_assert(TILE >= 2 * WM * BN, "reduction scratch must fit in the tile LDS");
    __shared__ __attribute__((aligned(16))) float smem[SM];
    float* As = smem;
    float* Bs = smem + KT * PA;
    float* wS = smem + ((TILE + 3) & ~3);
    int32_t* ptS = reinterpret_cast<int32_t*>(wS + BM);
    float* sv = wS + 2 * BM;
    float* tv = sv + VMAX;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = blockIdx.z;
    const int zoff = gr.aoff[g], n_out = gr.nout[g], ooff = gr.ooff[g];
    const float* Wg = W + gr.woff[g];
    const int n0 = blockIdx.y * BN;
    if (n0 >= n_out) return;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if ((int)(blockIdx.x * BM) >= n_rows) return;          // idle block (grid sized for the worst case)
    const int nk = (Kp + KT - 1) / KT;
    const int bulk = XM == 0 ? x.c_in : x.feat_c;

    float csum[TN], csq[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) { csum[t] = 0.f; csq[t] = 0.f; }

    int row0 = blockIdx.x * BM;
    XRaw ra[UA];
    float4 rb[UB];
    auto load_tile = [&](int kt) {
        const int k0 = kt * KT;
        const bool tail = k0 + KT > bulk;
#pragma unroll
        for (int it = 0; it < UA; ++it) {
            int i, kk; unit_T<BM>(it * 256 + tid, i, kk);
            const int r = row0 + i;
            const bool ok = r < n_rows && (k0 + kk < Kp);
            ra[it] = x_raw<XM>(x, r, ok, zoff, k0 + kk, tail, XM == 1 ? ptS[i] : 0);
        }
#pragma unroll
        for (int it = 0; it < UB; ++it) {
            int j, kk; unit_T<BN>(it * 256 + tid, j, kk);
            const int n = n0 + j;
            const bool ok = n < n_out && (k0 + kk < Kp);
            rb[it] = ldg4(Wg + (size_t)(ok ? n : 0) * Kp + (ok ? k0 + kk : 0));
        }
    };
    auto store_tile = [&](int kt) {
        const int k0 = kt * KT;
#pragma unroll
        for (int it = 0; it < UA; ++it) {
            int i, kk; unit_T<BM>(it * 256 + tid, i, kk);
            const int r = row0 + i;
            const bool ok = r < n_rows && (k0 + kk < Kp);
            store_T<BM>(As, i, kk, x_finish<XM>(x, ra[it], ok, k0 + kk, sv, tv));
        }
#pragma unroll
        for (int it = 0; it < UB; ++it) {
            int j, kk; unit_T<BN>(it * 256 + tid, j, kk);
            const bool ok = (n0 + j) < n_out && (k0 + kk < Kp);
            store_T<BN>(Bs, j, kk, f4sel(ok, rb[it], f4zero()));
        }
    };
    // ACT input: the first K-tile's loads need neither the row weights nor the BatchNorm vectors -- issue them first so
    // the three global-load latencies of the prologue (tile, vectors, weights) overlap instead of chaining
    bool preloaded = false;
    if (XM == 0) { load_tile(0); preloaded = true; }
    if (XM == 0 && x.affine) stage_affine<256>(sv, tv, x, zoff, x.c_in);
    for (; row0 < n_rows; row0 += gridDim.x * BM) {
        f32x16 acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
        if (tid < BM) {
            const int r = row0 + tid;
            wS[tid] = r < n_rows ? (row_w ? row_w[r] : 1.f) : 0.f;
            if (XM == 1) ptS[tid] = r < n_rows ? x.row_pt[r] : 0;
        }
        // fused max-pool: the row -> group map of this tile and of its two outside neighbours, the column's sign -- issued
        // here so that their latency sits under the K loop
        int pgl = -1, pg_before = -1, pg_after = -1;
        float psgn = 1.f;
        if (POOL) {
            const int r = row0 + lane;
            pgl = r < n_rows ? pe.row_grp[r] : -1;
            pg_before = row0 > 0 ? pe.row_grp[row0 - 1] : -1;
            pg_after = row0 + BM < n_rows ? pe.row_grp[row0 + BM] : -1;
            psgn = pe.gamma[n0 + lane] < 0.f ? -1.f : 1.f;
        }
        __syncthreads();                                   // wS / ptS / sv / tv visible
        if (!preloaded) load_tile(0);
        preloaded = false;
        for (int kt = 0; kt < nk; ++kt) {
            store_tile(kt);
            __syncthreads();
            if (kt + 1 < nk) load_tile(kt + 1);
            mfma_ktile<TM, TN, PA, PB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
            __syncthreads();
        }
        const int l31 = lane & 31, half = lane >> 5;
        if (POOL) {                                          // (64 x 64 tiles, one group, n_out % 64 == 0: the launcher checks)
            static_assert(!POOL || (BM == 64 && BN == 64 && TM == 1 && TN == 1 && TILE >= 64 * 65), "pooled epilogue: 64 x 64 tiles");
            float* zt = smem;                                // the operand tiles are done with (barrier at the end of the K loop)
#pragma unroll
            for (int v = 0; v < 16; ++v) zt[(wm * 32 + acc_row(v, half)) * 65 + wn * 32 + l31] = acc[0][0][v];
            __syncthreads();
            // lane = column; the tile's groups dealt to the four wavefronts
            {
                const float sg1[1] = {psgn};
                pool_tile64<1>(zt + lane, 65, 0, pgl, row0, min(64, n_rows - row0), sg1, __builtin_amdgcn_readfirstlane(wave), 4,
                               __builtin_amdgcn_readfirstlane(pg_before), __builtin_amdgcn_readfirstlane(pg_after),
                               pe.key + n0 + lane, pe.C);
            }
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * TN * 32 + tn * 32 + l31;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int il = wm * TM * 32 + tm * 32 + acc_row(v, half);
                    const int r = row0 + il;
                    const float zv = acc[tm][tn][v];
                    if (zout && r < n_rows && n < n_out) zout[(size_t)r * zout_pitch + ooff + n] = zv;
                    const float w = wS[il];
                    s1 = fmaf(w, zv, s1);
                    s2 = fmaf(w * zv, zv, s2);
                }
            csum[tn] += s1;
            csq[tn] += s2;
        }
        __syncthreads();   // wS / ptS reuse
    }
    if (stat_sum) {
        const int rep = DET ? blockIdx.x : blockIdx.x % GAD_STAT_REPLICAS;
        block_column_atomics<WM, WN, TN, DET>(smem, csum, csq, lane, wm, wn, n0, n_out,
                                              stat_sum + (size_t)rep * stat_stride + ooff,
                                              stat_sq + (size_t)rep * stat_stride + ooff);
    }
}
// ------------------------------------------------------------------------------------------------
// wide-tile forward for the MID-SIZE layers (SA2 / SA3 layers 2 and 3: 8e3 - 3e4 rows, K 128 - 256, 128 - 512 outputs).
// The 64 x 64 kernel above gives every wavefront ONE 32 x 32 accumulator: 16 MFMAs (0.45 us) per K-tile against ~1 us of
// global-load latency, a transposing LDS store of four ds_write_b32 per staged float4 and ~10 vector instructions per MFMA.
// Here a workgroup owns 64 rows x 128 columns, a wavefront 32 x 64 (two accumulators sharing the A fragment):
//   * 32 MFMAs (0.85 us) per K-tile and wavefront cover the load latency of the next tile (register-staged, issued right
//     after the previous LDS write), LDS is double-buffered: ONE barrier per K-tile;
//   * operands sit row-major in LDS, [row][32 + 4] floats: the staged float4 goes out as one ds_write_b128 (eight lanes
//     fill one row: conflict-free), fragments come in as one ds_read_b128 per four MFMA steps (k visited as 8j + 4h + i, the
//     streaming kernels' order: the 36-float pitch spreads 16 rows over all 64 banks);
//   * relu(scale * z + shift) is applied once per staged element, not per fragment read.
// XM = 1: the first layer of SA2 / SA3, whose input rows are GATHERED ([feat[pt] | src_xyz[pt] - ctr_xyz[grp]], features a
// multiple of 32 wide, already activated): the K loop runs over the feature columns only, the three coordinate columns
// are a rank-3 update of the accumulators in the epilogue (z += dx . W[n][feat_c .. feat_c + 2]) instead of a fifth,
// almost empty K-tile.
// Measured alone (tools/diag_gemm.py, B = 256 shapes): see profiles/README.md round 3.
// ------------------------------------------------------------------------------------------------
// SP: the products as split-bf16 MFMAs (namespace spw of gemm_common.hpp): A is split while it is staged, B comes from the layer's forward
// weight mirror (wsp: three planes of wsp_plane bf16, rows of wsp_pitch), same tiles, prologue and epilogue.
template <int XM, bool POOL, bool SP = false>
__global__ __launch_bounds__(256, 2) void gemm_fwd_wide_kernel(XSrc x, const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                               const float* __restrict__ row_w, const float* __restrict__ W,
                                                               int Kp, int n_out, float* __restrict__ zout, int zout_pitch,
                                                               double* __restrict__ stat_sum, double* __restrict__ stat_sq,
                                                               int stat_stride, PoolEpi pe, const uint16_t* __restrict__ wsp,
                                                               int wsp_pitch, int wsp_plane, unsigned long long* __restrict__ ts) {
    KTimer kt_(ts);
    GAD_WPH_DECL;
    GAD_WKL_DECL;
    constexpr int BM = 64, BN = 128, P = KT + 4, STAGE = SP ? spw::STAGE / 4 : (BM + BN) * P, VM = 512;
    static_assert(2 * STAGE >= 64 * 129, "the pooled epilogue's tile lives in the operand buffers");
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + 2 * VM + BM + 4 * BM];
    float* sv = smem + 2 * STAGE;
    float* tv = sv + VM;
    float* wS = tv + VM;
    float* dxS = wS + BM;                                // XM = 1: [row][4] = src_xyz[pt] - ctr_xyz[grp]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.y * BN;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if ((int)(blockIdx.x * BM) >= n_rows) return;
    const int nk = (XM == 0 ? Kp : x.feat_c) / KT;
    const int c4 = (tid & 7) * 4;                        // this thread's 16-byte column chunk inside a K-tile
    const int ur = tid >> 3;                             // ... and row (A: rows ur, ur + 32; B: ur, +32, +64, +96)
    // operands and output through buffer descriptors: a 32-bit byte offset per lane (set up once per row tile) + a scalar
    // offset per access instead of 64-bit pointer arithmetic per load / store; the output descriptor is bounded by the live
    // rows (a NULL zout: zero records), so stores of rows past them -- or of a pass that keeps no raw output -- are dropped
    const __amdgpu_buffer_rsrc_t ar_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(XM == 0 ? x.zin : x.feat), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, GAD_BUF_MAX, 0x00020000);
    const int zo_pitch4 = zout_pitch * 4;
    const __amdgpu_buffer_rsrc_t zo_ = __builtin_amdgcn_make_buffer_rsrc(zout ? zout : const_cast<float*>(W), 0, zout ? gad_nbytes(n_rows, zo_pitch4) : 0, 0x00020000);
    int vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vb[u] = ((n0 + ur + 32 * u) * Kp + c4) * 4;
    // SP: the weight mirror's rows n0 + (tid >> 2) + 64 u, 16-byte chunk tid & 3 of a K-tile's 64 bytes
    const __amdgpu_buffer_rsrc_t ws_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(SP ? wsp : reinterpret_cast<const uint16_t*>(W)), 0, GAD_BUF_MAX, 0x00020000);
    int vbs[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) vbs[u] = ((n0 + (tid >> 2) + 64 * u) * wsp_pitch + (tid & 3) * 8) * 2;
    unsigned char* const smem_b = reinterpret_cast<unsigned char*>(smem);
    const int sp_fo = ((half ^ ((l31 >> 2) & 3)) << 4);
    if (XM == 0) {
        if (x.bn.stat_sum) {
            // the input layer's train-mode BatchNorm finalised here (no gad_bn_finalize launch between the two GEMMs): every
            // workgroup forms scale / shift of the K input channels from the f64 statistics -- 16 loads per channel, in flight
            // beside the first K-tile's operand loads below -- and the first workgroup publishes them for the backward pass
            const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
            for (int i = tid; i < Kp; i += 256) {
                float sc, sh;
                gad_bn_fin_channel(x.bn, i, writer, sc, sh);
                sv[i] = sc; tv[i] = sh;
            }
        } else {
            stage_affine<256>(sv, tv, x, 0, Kp);
        }
    }

    float csum[2] = {0.f, 0.f}, csq[2] = {0.f, 0.f};
    for (int row0 = blockIdx.x * BM; row0 < n_rows; row0 += gridDim.x * BM) {
        f32x16 acc[2];
        f32x16 an[2];                                    // SP: the negated accumulators (odd k16-steps)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[t][v] = 0.f; if (SP) an[t][v] = 0.f; }
        int pgl = -1, pg_before = -1, pg_after = -1;
        float psgn[2] = {1.f, 1.f};
        if (POOL) {
            const int r = row0 + lane;
            pgl = r < n_rows ? pe.row_grp[r] : -1;
            pg_before = row0 > 0 ? pe.row_grp[row0 - 1] : -1;
            pg_after = row0 + BM < n_rows ? pe.row_grp[row0 + BM] : -1;
            psgn[0] = pe.gamma[n0 + lane] < 0.f ? -1.f : 1.f;
            psgn[1] = pe.gamma[n0 + 64 + lane] < 0.f ? -1.f : 1.f;
        }
        // rows past the live count are clamped to the last live row (never stored, weight 0 in the statistics)
        const int ra0 = min(row0 + ur, max(n_rows - 1, 0)), ra1 = min(row0 + ur + 32, max(n_rows - 1, 0));
        const int va0 = ((XM == 0 ? ra0 * x.zin_pitch : x.row_pt[ra0] * x.feat_c) + c4) * 4;
        const int va1 = ((XM == 0 ? ra1 * x.zin_pitch : x.row_pt[ra1] * x.feat_c) + c4) * 4;
        // two register sets: the global loads of a K-tile are issued TWO tiles before its LDS write (one tile of MFMAs is
        // ~0.85 us, less than the memory latency under load: with one set every K-tile's barrier waited for its loads)
        float4 ra2[2][2], rb2[2][SP ? 1 : 4];
        spw::BRegs rbs[SP ? 2 : 1];
        auto load_regs = [&](int kt, auto setc) {
            constexpr int S = decltype(setc)::value;
            const int k0 = kt * (KT * 4);
            ra2[S][0] = buf_ld4(ar_, va0, k0); ra2[S][1] = buf_ld4(ar_, va1, k0);
            if (SP) { spw::load_b(rbs[SP ? S : 0], ws_, vbs, wsp_plane * 2, kt); return; }
#pragma unroll
            for (int u = 0; u < (SP ? 1 : 4); ++u) rb2[S][u] = buf_ld4(wr_, vb[u], k0);
        };
        auto write_lds = [&](int kt, auto setc) {
            constexpr int S = decltype(setc)::value;
            const float4* ra = ra2[S];
            const float4* rb = rb2[S];
            float* As = smem + (kt & 1) * STAGE;
            float* Bs = As + BM * P;
            float4 s4 = make_float4(1.f, 1.f, 1.f, 1.f), t4 = f4zero();
            if (XM == 0) {
                s4 = *reinterpret_cast<const float4*>(sv + kt * KT + c4);
                t4 = *reinterpret_cast<const float4*>(tv + kt * KT + c4);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float4 v = ra[u];
                if (XM == 0) {
                    v.x = fmaxf(fmaf(v.x, s4.x, t4.x), 0.f); v.y = fmaxf(fmaf(v.y, s4.y, t4.y), 0.f);
                    v.z = fmaxf(fmaf(v.z, s4.z, t4.z), 0.f); v.w = fmaxf(fmaf(v.w, s4.w, t4.w), 0.f);
                }
                if (SP) spw::store_a4(smem_b + (kt & 1) * spw::STAGE, ur + 32 * u, tid, v, (ur & 1) ? 0x80000000u : 0u);
                else *reinterpret_cast<float4*>(As + (ur + 32 * u) * P + c4) = v;
            }
            if (SP) { spw::store_b(smem_b + (kt & 1) * spw::STAGE, rbs[SP ? S : 0], tid); return; }
#pragma unroll
            for (int u = 0; u < (SP ? 1 : 4); ++u) *reinterpret_cast<float4*>(Bs + (ur + 32 * u) * P + c4) = rb[u];
        };
        const std::integral_constant<int, 0> S0;
        const std::integral_constant<int, 1> S1;
        load_regs(0, S0);
        if (nk > 1) load_regs(1, S1);
        __syncthreads();                                 // sv / tv visible; the previous row tile's LDS reads (wS, zt) are done
        if (tid < BM) {
            const int r = row0 + tid;
            wS[tid] = r < n_rows ? (row_w ? row_w[r] : 1.f) : 0.f;
            if (XM == 1) {                               // the row's recentred coordinates (rounded as the oracle rounds them)
                const int rr = min(r, max(n_rows - 1, 0));
                const float* p = x.src_xyz + (size_t)x.row_pt[rr] * 3;
                float q0 = p[0], q1 = p[1], q2 = p[2];
                if (x.ctr_xyz) {
                    const float* cp = x.ctr_xyz + (size_t)x.row_grp[rr] * 3;
                    q0 = __fsub_rn(q0, cp[0]); q1 = __fsub_rn(q1, cp[1]); q2 = __fsub_rn(q2, cp[2]);
                }
                *reinterpret_cast<float4*>(dxS + 4 * tid) = make_float4(q0, q1, q2, 0.f);
            }
        }
        GAD_WPH(1);
        write_lds(0, S0);
        if (nk > 2) load_regs(2, S0);
        __syncthreads();
        GAD_WPH(2);
        auto ktile = [&](int kt, auto nxtc) {             // MFMAs of tile kt; tile kt + 1 (register set nxtc) -> LDS; loads of kt + 3
            if (SP) {
                GAD_WKL(0);
                spw::ktile(smem_b + (kt & 1) * spw::STAGE, (wm * 32 + l31) * 64, (wn * 64 + l31) * 64, sp_fo, acc, an);
                GAD_WKL(1);
                if (kt + 1 < nk) write_lds(kt + 1, nxtc);
                if (kt + 3 < nk) load_regs(kt + 3, nxtc);
                GAD_WKL(2);
                __syncthreads();
                GAD_WKL(3);
                return;
            }
            const float* As = smem + (kt & 1) * STAGE + (wm * 32 + l31) * P + 4 * half;
            const float* Bs = smem + (kt & 1) * STAGE + BM * P + (wn * 64 + l31) * P + 4 * half;
            float4 a4 = *reinterpret_cast<const float4*>(As);
            float4 b0 = *reinterpret_cast<const float4*>(Bs), b1 = *reinterpret_cast<const float4*>(Bs + 32 * P);
#pragma unroll
            for (int j = 0; j < KT / 8; ++j) {
                float4 an = a4, bn0 = b0, bn1 = b1;
                if (j + 1 < KT / 8) {                    // next k group's fragments land under this group's MFMAs
                    an = *reinterpret_cast<const float4*>(As + 8 * (j + 1));
                    bn0 = *reinterpret_cast<const float4*>(Bs + 8 * (j + 1));
                    bn1 = *reinterpret_cast<const float4*>(Bs + 32 * P + 8 * (j + 1));
                }
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b1.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b0.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b0.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b1.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b1.w, acc[1], 0, 0, 0);
                a4 = an; b0 = bn0; b1 = bn1;
            }
            if (kt + 1 < nk) write_lds(kt + 1, nxtc);    // the other LDS buffer: its readers passed the previous barrier
            if (kt + 3 < nk) load_regs(kt + 3, nxtc);
            __syncthreads();
        };
        for (int kt = 0; kt < nk; kt += 2) {             // (nk is even: K is a multiple of 64 here)
            ktile(kt, S1);
            if (kt + 1 < nk) ktile(kt + 1, S0);
        }
        GAD_WPH(3);
        if (SP) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][v] = (v & 1) ? an[t][v] - acc[t][v] : acc[t][v] - an[t][v];   // (odd rows entered negated)
        }
        if (XM == 1) {                                   // the three coordinate columns: z += dx . W[n][feat_c .. feat_c + 2]
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float* wx = W + (size_t)(n0 + wn * 64 + t * 32 + l31) * Kp + x.feat_c;
                const float w0 = wx[0], w1 = wx[1], w2 = wx[2];
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float4 q = *reinterpret_cast<const float4*>(dxS + 4 * (wm * 32 + acc_row(v, half)));
                    acc[t][v] = fmaf(q.x, w0, fmaf(q.y, w1, fmaf(q.z, w2, acc[t][v])));
                }
            }
        }
        if (POOL) {
            float* zt = smem;                            // [64][129]: every wavefront is past the K loop's last barrier
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) zt[(wm * 32 + acc_row(v, half)) * 129 + wn * 64 + t * 32 + l31] = acc[t][v];
            __syncthreads();
            const int gb = __builtin_amdgcn_readfirstlane(pg_before), ga = __builtin_amdgcn_readfirstlane(pg_after);
            pool_tile64<2>(zt + lane, 129, 64, pgl, row0, min(64, n_rows - row0), psgn, wave, 4, gb, ga, pe.key + n0 + lane, pe.C);
        }
        if (SP) {
            // stores first, then the statistics from ONE batch of weight reads.  (Interleaved as in the FP32 path below, hipcc
            // packs the two column tiles into v_pk_* pairs and refills the weight registers piecemeal -- ds_read_b96 / b32 / b64
            // into registers whose stores are still in flight; with two workgroups per CU that form produced wrong sums of
            // squares for the first column tile in 29 of 40 launches on an MI355X, this one in 0 of 40: tools/diag_split_sq.py.)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = n0 + wn * 64 + t * 32 + l31;
            const int vzo = (4 * half * zout_pitch + n) * 4;
#pragma unroll
            for (int v = 0; v < 16; ++v)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[t][v]), zo_, vzo, (row0 + wm * 32 + (v & 3) + 8 * (v >> 2)) * zo_pitch4, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float w = wS[wm * 32 + acc_row(v, half)];
                const float zv = acc[t][v];
                s1 = fmaf(w, zv, s1);
                s2 = fmaf(w * zv, zv, s2);
            }
            csum[t] += s1;
            csq[t] += s2;
        }
        } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = n0 + wn * 64 + t * 32 + l31;
            const int vzo = (4 * half * zout_pitch + n) * 4;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int il = wm * 32 + acc_row(v, half);
                const float zv = acc[t][v];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(zv), zo_, vzo, (row0 + wm * 32 + (v & 3) + 8 * (v >> 2)) * zo_pitch4, 0);
                const float w = wS[il];
                s1 = fmaf(w, zv, s1);
                s2 = fmaf(w * zv, zv, s2);
            }
            csum[t] += s1;
            csq[t] += s2;
        }
        }
        // (the next row tile's first barrier orders these wS / zt reads before its writes)
        GAD_WPH(4);
    }
    if (stat_sum) {
        const int rep = blockIdx.x % GAD_STAT_REPLICAS;
        block_column_atomics<2, 2, 2>(smem, csum, csq, lane, wm, wn, n0, n_out, stat_sum + (size_t)rep * stat_stride,
                                      stat_sq + (size_t)rep * stat_stride);
    }
#ifdef GAD_W_PHASES
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GAD_WPH(5);
    GAD_WPH_STORE(ts);
    GAD_WKL_STORE(ts);
#endif
}

// the wide-tile kernel covers: ACT input, one group, K = the channel count itself (a multiple of 32, no bias / extra
// column), outputs a multiple of 128
static bool fwd_wideable(const gad_gemm_fwd_args& a) {
    if (g_opt.deterministic || !g_opt.fwd_wide || a.n_groups != 1 || a.zin_off[0] != 0 || a.w_off[0] != 0 || a.out_off[0] != 0) return false;
    // (gathered input: the point-major feature tensor has at most as many rows as there are (group, point) rows upstream)
    if (!fits_i32_bytes(a.n_rows, a.mode == 1 ? a.feat_c : a.zin_pitch, a.zout ? a.zout_pitch : 0, 0, 0)) return false;
    if (a.n_rows < 2048 || a.n_out[0] % 128 != 0 || a.ones_col >= 0) return false;
    if (a.mode == 2) return false;
    if (a.mode == 1)                                     // gathered first layer: features a multiple of 32, + 3 coordinates
        return g_opt.fwd_wide != 2 && !a.pool_key && a.act_c == 0 && a.feat_c % 32 == 0 && a.feat_c >= 32 && a.feat_c <= 512 &&
               a.Kp == ((a.feat_c + 3 + 7) & ~7);
    if (a.Kp % 32 != 0 || a.Kp > 512 || a.Kp != a.c_in) return false;
    return !a.extra && a.scale && a.shift && a.relu;
}

// ------------------------------------------------------------------------------------------------
// streaming forward for the wide-and-shallow SA1 layers (rows ~ 2e5, Kp <= 64, n_out <= 128):
// HBM-bound (SA1 layer 3: 192 B/row moved vs 16 kFLOP/row), so the kernel is built around bytes in
// flight rather than around a block tile:
//   * W (<= 34 KB) is staged ONCE per workgroup in LDS, row-major [n][Kp+4] (ds_read_b128, conflict-free);
//   * every wavefront owns 32-row slabs: lane (r = lane%32, h = lane/32) loads X[r][8j+4h..+3] as 16-byte
//     loads straight into the MFMA A-operand registers (no LDS round trip, no workgroup barrier in the
//     loop) -- the reduction index is visited in the order k = 8j+4h+i, identically for A and B;
//   * the next slab's loads are issued before the current slab's MFMAs (register double buffer) and the
//     grid is persistent at 2 wavefronts per SIMD, so loads, MFMAs and the epilogue stores of different
//     wavefronts overlap.
// ------------------------------------------------------------------------------------------------
// NOTE (measured, tools/ubench/mfma_valu.hip): on gfx950 the f32 MFMA shares the vector ALU -- every VALU
// instruction issued between MFMAs adds its ~4 clocks to the 64 of the MFMA, also with 2 wavefronts per SIMD.
// So the loop below is written for a minimal VALU instruction count: packed (2-wide) f32 math for the BatchNorm
// affine and the statistics, buffer stores whose row offset lives in an SGPR (no per-store address arithmetic),
// clamped row indices instead of per-element selects.
// XM = 2 / 3 (round 4): the 64-channel ACT input is not read but RECOMPUTED per slab from the gathered rows of
// the stage's first layer (packed K = 8 / 16: XM - 1 k groups) -- z1^T = W1 . X^T with the operands of the first layer's own
// MFMAs swapped, so the accumulator registers of lane (row, half) ARE this kernel's A fragments (channels 8j + 4 half + i) and
// every product and sum is the one the first layer's launch made (bit-equal z1): 8 / 16 extra MFMAs per slab instead of
// 8 KB of z1 from HBM.  The first layer's launch still provides the BatchNorm statistics (and z1 for a pass that is
// back-propagated).
template <int KJ, int TN, int XM, bool POOL, bool SP = false>
__global__ __launch_bounds__(512, 2) void gemm_fwd_stream_kernel(XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                                  int n_rows_static, const float* __restrict__ row_w,
                                                                  const float* __restrict__ W, float* __restrict__ zout,
                                                                  double* __restrict__ stat_sum,
                                                                  double* __restrict__ stat_sq, int stat_stride, PoolEpi pe,
                                                                  unsigned long long* __restrict__ ts) {
#ifdef GAD_X_PHASES
    const long long kt_start = __builtin_readcyclecounter();
#else
    KTimer kt(ts);
#endif
    constexpr int KP = 8 * KJ, NO = 32 * TN, PW = KP + 4;
    constexpr bool RE = XM >= 2;                         // recomputed ACT input
    constexpr int PK = RE ? XM - 1 : 0;                  // k groups of the recomputed first layer
    constexpr bool ACT = XM == 0 || RE, GATHER = XM == 1 || RE;
    constexpr int NG = RE ? PK : KJ;                     // k groups a slab's loads cover
    static_assert(!RE || (KJ == 8 && !POOL), "recomputed input: 64 channels");
    // SP (opt-in split-bf16 arithmetic, ACT input with 64 channels): W lives in LDS as three bf16 planes [plane][n][64 (+ 8 pad)] and a
    // lane's slab columns are 16 s + 8 half + 0 .. 7 (the A layout of v_mfma_f32_32x32x16_bf16) instead of 8 j + 4 half + 0 .. 3
    static_assert(!SP || (XM == 0 && KJ == 8), "split-bf16: ACT input, 64 channels");
    constexpr int PB = 2 * KP + 16;                      // bytes per row of a bf16 plane
    __shared__ __attribute__((aligned(16))) float Ws[SP ? 3 * NO * PB / 4 : NO * PW];
    __shared__ __attribute__((aligned(16))) float sv[KP], tv[KP];
    __shared__ float red[2 * 8 * NO];
    __shared__ float pz[POOL ? 8 * 32 * 64 : 1];        // fused max-pool: a 32-row x 64-column tile per wavefront
    static_assert(!POOL || TN == 4, "pooled epilogue: 128 output columns");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    const int n_slabs = (n_rows + 31) >> 5;
#if GAD_X_PHASES == 2
    long long st1, st2, st3, st4;
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    GAD_PH_STAMP(st1);                                   // the live row count has arrived
#endif
    // 8 wavefronts per workgroup, one workgroup per CU: wavefronts w and w+4 share a SIMD (cyclic placement).  Slabs
    // are dealt wave-major (w * gridDim + block), so the left-over slabs of the last round go to w = 0..3 first and
    // every SIMD ends up with the same slab count +-1 (dealing block-major left whole CUs a round short: -20 %).
    int stride = gridDim.x * 8;
    int slab = wave * gridDim.x + blockIdx.x;            // wave-uniform (SGPR)
    int slab_end = n_slabs;
    if (POOL) {
        // fused max-pool: every wavefront walks a CONTIGUOUS range of slabs, so a group's running maximum is carried in
        // registers from slab to slab and only the two groups cut by the range's ends need atomics (same slab count per
        // wavefront +-1 as the dealing above)
        const int nw = gridDim.x * 8, base = n_slabs / nw, rem = n_slabs - base * nw;
        slab_end = slab * base + min(slab, rem) + base + (slab < rem ? 1 : 0);
        slab = slab * base + min(slab, rem);
        stride = 1;
    }
    // output through a buffer descriptor: rows >= n_rows fall outside num_records and are dropped by the hardware
    const bool store_z = zout != nullptr;                // (a pass that is never back-propagated keeps only the pooled maxima)
    const __amdgpu_buffer_rsrc_t zrsrc =
        __builtin_amdgcn_make_buffer_rsrc(store_z ? zout : const_cast<float*>(W), 0, store_z ? gad_nbytes(n_rows, NO * 4) : 0, 0x00020000);
    const int zlane = (4 * half * NO + l31) * 4;         // byte offset of (row 4*half, column l31)
    // fused max-pool: in the scan a lane owns columns lane and 64 + lane; +-1 = the sign of their BatchNorm weight
    float psgn[2];
    PoolRun prun[2];
    const int range0 = slab * 32;
    int g_after = -1;                                    // group of the first row after the range (-1: none)
    if (POOL && slab < slab_end) {
        const int g0 = pe.row_grp[range0];               // (range0 < n_rows: the range has rows)
        const int part0 = range0 > 0 && pe.row_grp[range0 - 1] == g0;
        if (slab_end * 32 < n_rows) g_after = pe.row_grp[slab_end * 32];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            psgn[p] = pe.gamma[p * 64 + lane] < 0.f ? -1.f : 1.f;
            prun[p].g = g0; prun[p].part = part0; prun[p].v = -INFINITY; prun[p].row = range0;
        }
    }

    f32x2 csum[TN], csq[TN];                             // .x/.y: even / odd accumulator rows, summed at the end
#pragma unroll
    for (int t = 0; t < TN; ++t) { csum[t] = f32x2{0.f, 0.f}; csq[t] = f32x2{0.f, 0.f}; }

    XRaw ra[NG], rn[NG];
    float4 w1f[RE ? 2 : 1][RE ? PK : 1];                 // recomputed input: W1[32 b + l31][8 j + 4 half .. + 3], loop-invariant
    if (RE) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int j = 0; j < PK; ++j) w1f[b][j] = ldg4(x.pre_W + (size_t)(32 * b + l31) * x.pre_Kp + 8 * j + 4 * half);
    }
    int pt_nxt = 0;
    auto load_pt = [&](int sl) {          // point index of the lane's row in slab sl (gather input only)
        const int r = min(sl * 32 + l31, max(n_rows - 1, 0));
        return (GATHER && sl < n_slabs) ? x.row_pt[r] : 0;
    };
    auto load_slab = [&](int sl, int pt, XRaw (&dst)[NG]) {
        const int r = min(sl < n_slabs ? sl * 32 + l31 : 0, max(n_rows - 1, 0));      // clamped: ragged rows repeat the last row
        if (GATHER) {
            // SA1's gathered rows [f (4) | x_j - c_i (3) | action (0 / 6)]: everything a row needs in FIVE loads (features,
            // point, centre as 12-byte loads, action as two), then each (k group, half) picks its four columns.  x_raw per
            // k group issued 11 scalar gathers per lane, most of them for columns the lane does not feed: the layer was
            // bound by the texture path (64 cache lines per gather instruction), not by its 54 MB of output.
            struct F3 { float x, y, z; } __attribute__((packed, aligned(4)));
            const float4 f = ldg4(x.feat + (size_t)pt * 4);
            const F3 p = *reinterpret_cast<const F3*>(x.src_xyz + (size_t)pt * 3);
            const int grp = x.row_grp[r];
            float q0 = p.x, q1 = p.y, q2 = p.z;
            if (x.ctr_xyz) {
                const F3 c = *reinterpret_cast<const F3*>(x.ctr_xyz + (size_t)grp * 3);
                q0 = __fsub_rn(q0, c.x); q1 = __fsub_rn(q1, c.y); q2 = __fsub_rn(q2, c.z);
            }
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f;
            if (x.action) {                                                  // (fwd_streamable: act_c == 6)
                const float* ap = x.action + (size_t)(grp / x.gps) * 6;
                const F3 u = *reinterpret_cast<const F3*>(ap), v = *reinterpret_cast<const F3*>(ap + 3);
                a0 = u.x; a1 = u.y; a2 = u.z; a3 = v.x; a4 = v.y; a5 = v.z;
            }
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                dst[j].a = f;
                if (j == 0) dst[j].s = make_float4(q0, q1, q2, a0);          // columns 4 .. 7 (half 1; half 0 takes the features)
                else dst[j].s = half ? make_float4(a5, 0.f, 0.f, 0.f) : make_float4(a1, a2, a3, a4);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NG; ++j)
            dst[j] = x_raw<GATHER ? 1 : 0>(x, r, true, 0, SP ? 16 * (j >> 1) + 8 * half + 4 * (j & 1) : 8 * j + 4 * half, GATHER, pt);
    };
    auto lds_b = [&](int j, float4 (&b4)[TN]) {
#pragma unroll
        for (int t = 0; t < TN; ++t) b4[t] = *reinterpret_cast<const float4*>(Ws + (t * 32 + l31) * PW + 8 * j + 4 * half);
    };
    {   // the first slab's loads are in flight while W and the input layer's affine are staged
        const int pt0 = load_pt(slab);
        load_slab(slab, pt0, ra);
        pt_nxt = load_pt(slab + stride);
    }
    {   // stage W: all 16-byte loads in flight before the first LDS store; the input layer's per-channel affine (published vectors,
        // or its BatchNorm finalised here from the statistic replicas -- see gemm_fwd_wide_kernel) is fetched UNDER the W loads:
        // one global round trip for the whole prologue instead of two
        constexpr int UNITS = NO * KJ * 2, UW = (UNITS + 511) / 512;
        float4 wr[UW];
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid;
            wr[it] = ldg4(W + (size_t)(u < UNITS ? u : 0) * 4);
        }
#if GAD_X_PHASES == 2
        GAD_PH_STAMP(st2);                               // first slab + W loads issued
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        GAD_PH_STAMP(st3);                               // ... and arrived
#endif
        if (ACT && tid < KP) {                            // (KP <= 64 < 512 threads: one channel per thread)
            float sc, sh;
            if (x.bn.stat_sum) gad_bn_fin_channel(x.bn, tid, blockIdx.x == 0, sc, sh);
            else { sc = x.scale[tid]; sh = x.shift[tid]; }
            sv[tid] = sc; tv[tid] = sh;
        }
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid;
            const int n = u / (KJ * 2), c = (u % (KJ * 2)) * 4;
            if (SP) {
                unsigned h0, m0, l0, h1, m1, l1;
                gad_split2(wr[it].x, wr[it].y, h0, m0, l0);
                gad_split2(wr[it].z, wr[it].w, h1, m1, l1);
                unsigned char* wp = reinterpret_cast<unsigned char*>(Ws) + n * PB + c * 2;
                if (u < UNITS) {
                    *reinterpret_cast<uint2*>(wp) = make_uint2(h0, h1);
                    *reinterpret_cast<uint2*>(wp + NO * PB) = make_uint2(m0, m1);
                    *reinterpret_cast<uint2*>(wp + 2 * NO * PB) = make_uint2(l0, l1);
                }
            } else if (u < UNITS) *reinterpret_cast<float4*>(Ws + n * PW + c) = wr[it];
        }
    }
    __syncthreads();
#if GAD_X_PHASES == 2
    GAD_PH_STAMP(st4);
    if (ts && lane == 0) {
        auto c16 = [&](long long t) { const long long d = (t - kt_start) >> 2; return (unsigned long long)(d > 65535 ? 65535 : d); };
        ts[2 * (blockIdx.x * 8 + wave)] = c16(st1) | (c16(st2) << 16) | (c16(st3) << 32) | (c16(st4) << 48);
    }
#endif

#ifdef GAD_X_PHASES
    long long tA = 0, tB = 0, tC = 0, ph_top = 0, ph_mfma = 0, ph_epi = 0;
    int ph_n = 0;
    long long tP, tS;
    GAD_PH_STAMP(tP);
    tS = (long long)kt_start;
#endif
    for (; slab < slab_end; slab += stride) {
        load_slab(slab + stride, pt_nxt, rn);
        pt_nxt = load_pt(slab + 2 * stride);
        // the 16 rows this lane owns in the accumulator layout: 4 runs of 4 consecutive rows -> 4 aligned loads
        float4 w4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r0 = slab * 32 + 8 * q + 4 * half;
            w4[q] = row_w ? ldg4(row_w + (r0 + 3 < n_rows_static ? r0 : 0)) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
        if (slab * 32 + 32 > n_rows) {                   // ragged last slab (wave-uniform branch): zero the missing rows
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float* wq = &w4[q].x;
#pragma unroll
                for (int e = 0; e < 4; ++e) wq[e] = (slab * 32 + 8 * q + 4 * half + e < n_rows) ? wq[e] : 0.f;
            }
        }
        int gl = -1;                                     // fused max-pool: lane i (both halves) holds the group of slab row i
        if (POOL) { const int rr = slab * 32 + l31; gl = rr < n_rows ? pe.row_grp[rr] : -1; }
        __asm__ volatile("" ::: "memory");        // keep the (loop-invariant) LDS reads of W inside the loop: registers
        f32x16 acc[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
        float4 bn[TN];
        if (!SP) lds_b(0, bn);
        GAD_PH_STAMP(tA);
        if (SP) {
            const unsigned char* wp = reinterpret_cast<const unsigned char*>(Ws) + l31 * PB + 16 * half;
            constexpr int NS = SP ? KJ / 2 : 1;           // 16-channel steps
            gad_u32x4 AH[NS], AM[NS], AL[NS];
#pragma unroll
            for (int sg = 0; sg < NS; ++sg) {
                unsigned ah[4], am[4], al[4];
#pragma unroll
                for (int e = 0; e < 2; ++e) {           // relu(scale * z + shift) of the lane's 8 channels, then hi / mid / lo
                    const int c = 16 * sg + 8 * half + 4 * e;
                    const float4 s4 = *reinterpret_cast<const float4*>(sv + c), t4 = *reinterpret_cast<const float4*>(tv + c);
                    const float4 zr = ra[SP ? 2 * sg + e : 0].a;
                    const float a0 = __builtin_fmaxf(fmaf(zr.x, s4.x, t4.x), 0.f), a1 = __builtin_fmaxf(fmaf(zr.y, s4.y, t4.y), 0.f);
                    const float a2 = __builtin_fmaxf(fmaf(zr.z, s4.z, t4.z), 0.f), a3 = __builtin_fmaxf(fmaf(zr.w, s4.w, t4.w), 0.f);
                    gad_split2(a0, a1, ah[2 * e], am[2 * e], al[2 * e]);
                    gad_split2(a2, a3, ah[2 * e + 1], am[2 * e + 1], al[2 * e + 1]);
                }
                // the bf16 MFMA's adder truncates toward -inf (a -1e-8 relative bias, tools/ubench/split_bf16.hip): odd steps
                // accumulate the NEGATED products into a second accumulator pair, the difference of the two cancels it
                const unsigned sgn = ((sg ^ l31) & 1) ? 0x80008000u : 0u;        // (and the whole of an odd row: see the header)
                AH[sg] = gad_u32x4{ah[0] ^ sgn, ah[1] ^ sgn, ah[2] ^ sgn, ah[3] ^ sgn};
                AM[sg] = gad_u32x4{am[0] ^ sgn, am[1] ^ sgn, am[2] ^ sgn, am[3] ^ sgn};
                AL[sg] = gad_u32x4{al[0] ^ sgn, al[1] ^ sgn, al[2] ^ sgn, al[3] ^ sgn};
            }
#pragma unroll
            for (int pp = 0; pp < TN / 2; ++pp) {        // two 32-column tiles at a time: (plain, negated) accumulator pairs
                f32x16 an[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int v = 0; v < 16; ++v) an[i][v] = 0.f;
#pragma unroll
                for (int sg = 0; sg < NS; ++sg) {
                    gad_u32x4 BH[2], BM[2], BL[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const unsigned char* q = wp + (2 * pp + i) * 32 * PB + 32 * sg;
                        BH[i] = *reinterpret_cast<const gad_u32x4*>(q);
                        BM[i] = *reinterpret_cast<const gad_u32x4*>(q + NO * PB);
                        BL[i] = *reinterpret_cast<const gad_u32x4*>(q + 2 * NO * PB);
                    }
                    // the six products of weight >= 2^-16, smallest first
#define GAD_SPLIT_MFMA(A, B)                                                                                                   \
                    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                             \
                        if (sg & 1) an[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A[sg]), gad_as_bf16x8(B[i]), an[i], 0, 0, 0); \
                        else acc[2 * pp + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A[sg]), gad_as_bf16x8(B[i]), acc[2 * pp + i], 0, 0, 0); \
                    }
                    GAD_SPLIT_MFMA(AL, BH) GAD_SPLIT_MFMA(AH, BL) GAD_SPLIT_MFMA(AM, BM)
                    GAD_SPLIT_MFMA(AM, BH) GAD_SPLIT_MFMA(AH, BM) GAD_SPLIT_MFMA(AH, BH)
#undef GAD_SPLIT_MFMA
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[2 * pp + i][v] = (v & 1) ? an[i][v] - acc[2 * pp + i][v] : acc[2 * pp + i][v] - an[i][v];
            }
        }
        f32x16 zacc[RE ? 2 : 1];
        if (RE) {                   // z1^T tile: channels 32 b + (accumulator row), rows = lanes; the first layer's own products
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int v = 0; v < 16; ++v) zacc[b][v] = 0.f;
#pragma unroll
            for (int j = 0; j < PK; ++j) {
                const float4 xb = x_finish<1>(x, ra[j], true, 8 * j + 4 * half, sv, tv);
#pragma unroll
                for (int b = 0; b < 2; ++b) zacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1f[b][j].x, xb.x, zacc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < 2; ++b) zacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1f[b][j].y, xb.y, zacc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < 2; ++b) zacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1f[b][j].z, xb.z, zacc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < 2; ++b) zacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1f[b][j].w, xb.w, zacc[b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < (SP ? 0 : KJ); ++j) {
            float4 b4[TN];
#pragma unroll
            for (int t = 0; t < TN; ++t) b4[t] = bn[t];
            float4 a4;
            if (ACT) {              // relu(scale * z + shift): two packed FMAs + four max
                const float4 s4 = *reinterpret_cast<const float4*>(sv + 8 * j + 4 * half);
                const float4 t4 = *reinterpret_cast<const float4*>(tv + 8 * j + 4 * half);
                float4 zr;
                if (RE) zr = make_float4(zacc[j >> 2][4 * (j & 3)], zacc[j >> 2][4 * (j & 3) + 1], zacc[j >> 2][4 * (j & 3) + 2],
                                         zacc[j >> 2][4 * (j & 3) + 3]);
                else zr = ra[RE ? 0 : j].a;
                const f32x2 lo = f32x2{zr.x, zr.y} * f32x2{s4.x, s4.y} + f32x2{t4.x, t4.y};
                const f32x2 hi = f32x2{zr.z, zr.w} * f32x2{s4.z, s4.w} + f32x2{t4.z, t4.w};
                a4 = make_float4(__builtin_fmaxf(lo.x, 0.f), __builtin_fmaxf(lo.y, 0.f), __builtin_fmaxf(hi.x, 0.f),
                                 __builtin_fmaxf(hi.y, 0.f));
            } else {
                a4 = x_finish<1>(x, ra[RE ? 0 : j], true, 8 * j + 4 * half, sv, tv);
            }
            if (j + 1 < KJ) lds_b(j + 1, bn);      // next group's fragments land under this group's MFMAs
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4[t].w, acc[t], 0, 0, 0);
        }
        GAD_PH_STAMP(tB);
        // epilogue: raw layer output (SGPR row offset + immediate column offset: no address arithmetic) and the
        // weighted BatchNorm partial sums, two accumulator rows per packed instruction
        const int zrow = slab * 32 * NO * 4;
        if (POOL) {
            // 64 columns at a time through this wavefront's LDS tile (in-order LDS: no barrier), then lane = column
            float* zt = pz + wave * (32 * 64);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    zt[acc_row(v, half) * 64 + l31] = acc[2 * p][v];
                    zt[acc_row(v, half) * 64 + 32 + l31] = acc[2 * p + 1][v];
                }
                pool_scan32(zt + lane, 64, gl, slab * 32, psgn[p], prun[p], pe.key + p * 64 + lane, pe.C);
            }
        }
#pragma unroll
        for (int v = 0; v < 16; v += 2) {
            const int rb = ((v & 3) + 8 * (v >> 2)) * NO * 4;
            const f32x2 wr = f32x2{(&w4[v >> 2].x)[v & 3], (&w4[v >> 2].x)[(v & 3) + 1]};
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const f32x2 zv = f32x2{acc[t][v], acc[t][v + 1]};
                if (store_z) {                           // (NULL zout: statistics / pooled maxima only; rows past n_rows are dropped)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[t][v]), zrsrc, zlane + t * 128, zrow + rb, GAD_STREAM_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[t][v + 1]), zrsrc, zlane + t * 128, zrow + rb + NO * 4, GAD_STREAM_STORE_AUX);
                }
                const f32x2 wz = wr * zv;
                csum[t] += wz;
                csq[t] += wz * zv;
            }
        }
#pragma unroll
        for (int j = 0; j < NG; ++j) ra[j] = rn[j];
#ifdef GAD_X_PHASES
        GAD_PH_STAMP(tC);
        ph_top += tA - tP; ph_mfma += tB - tA; ph_epi += tC - tB; tP = tC; ++ph_n;
#endif
    }
#ifdef GAD_X_PHASES
    if (ts && lane == 0) {
        const unsigned w = blockIdx.x * 8 + wave;
        if (GAD_X_PHASES != 2) ts[2 * w] = ((unsigned long long)ph_mfma << 32) | (unsigned long long)(ph_epi & 0xffffffffu);
        ts[2 * w + 1] = ((unsigned long long)ph_top << 32) | ((unsigned long long)(tP - tS) & 0xffffff00u) | (unsigned long long)ph_n;
    }
#endif
    if (POOL && range0 < slab_end * 32) {                // the group still open at the end of the range
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (prun[p].g >= 0)
                pool_put(pe.key + p * 64 + lane, prun[p].g, pe.C, prun[p].v, prun[p].row, prun[p].part != 0 || prun[p].g == g_after);
    }
    if (stat_sum) {
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const float c0 = csum[t].x + csum[t].y, c1 = csq[t].x + csq[t].y;
            const float s0 = c0 + __shfl_xor(c0, 32, 64);
            const float s1 = c1 + __shfl_xor(c1, 32, 64);
            if (lane < 32) { red[wave * NO + t * 32 + lane] = s0; red[(8 + wave) * NO + t * 32 + lane] = s1; }
        }
        __syncthreads();
        if (tid < NO) {
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) { s0 += red[w * NO + tid]; s1 += red[(8 + w) * NO + tid]; }
            const int rep = blockIdx.x % GAD_STAT_REPLICAS;
            atomic_add_f64(stat_sum + (size_t)rep * stat_stride + tid, (double)s0);
            atomic_add_f64(stat_sq + (size_t)rep * stat_stride + tid, (double)s1);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// skinny forward for the small-M layers (FC head and actor/critic heads: M = batch rows <= 1024, K up to 1032).
// A 64x64-tile launch has M/64 * N/64 = 32..64 workgroups for 256 CUs and walks K serially: 33 K-tiles of
// (global load -> LDS -> barrier -> 16 MFMA -> barrier) at ~1.2 us each (load latency, nothing to overlap with).
// Here every workgroup owns one 32x32 output tile and its 8 wavefronts split K: each wavefront issues ALL the
// 16-byte loads of its K slice (A and B operand straight in MFMA register layout, k visited as 8j+4h+i like the
// streaming kernel, no LDS staging, no barrier) before its first MFMA, so the load latency is paid about once;
// the partial tiles are summed through LDS.  256 rows x 1024 -> 512: 37.8 us -> see tools/diag_gemm.py.
// ------------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_fwd_skinny_kernel(XSrc x, Groups gr, int n_rows,
                                                                     const float* __restrict__ row_w,
                                                                     const float* __restrict__ W, int Kp,
                                                                     float* __restrict__ zout, int zout_pitch,
                                                                     double* __restrict__ stat_sum,
                                                                     double* __restrict__ stat_sq, int stat_stride, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    __shared__ __attribute__((aligned(16))) float stA[NW * 32 * SK_SP], stW[NW * 32 * SK_SP];
    __shared__ __attribute__((aligned(16))) float sv[SK_KCAP], tv[SK_KCAP];
    float* const part = stA;                                  // partial tiles reuse the operand stage: wavefront w's 4 KB inside its own 4.5 KB
    static_assert(32 * SK_SP >= 16 * 64, "partial tile must fit the wavefront's stage");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int g = blockIdx.z;
    const int zoff = gr.aoff[g], n_out = gr.nout[g], ooff = gr.ooff[g];
    // x = column tile, y = row tile: workgroups go to the 8 XCDs round-robin in x-fastest order, so the workgroups that read
    // one 32-column slice of W share an L2 (each XCD pulls 1/8 of the weights instead of all of them)
    const int n0 = blockIdx.x * 32, row0 = blockIdx.y * 32;
    if (n0 >= n_out) return;                                  // workgroup-uniform
    const float* Wg = W + gr.woff[g] + (size_t)min(n0 + l31, n_out - 1) * Kp + 4 * half;   // clamped: extra columns unused
    const int r = min(row0 + l31, max(n_rows - 1, 0));                // clamped: extra rows are neither stored nor counted
    const int nj = Kp >> 3;
    const int per = (nj + NW - 1) / NW;
    const int j0 = wave * per, j1 = min(nj, j0 + per);        // this wavefront's k groups (wave-uniform)

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    // Operand blocks of four k groups (32 columns) go through a wavefront-private LDS stage: loaded COALESCED (8 lanes per
    // 128-byte row segment, 8 rows per instruction: 8-16 cache lines instead of the 32 a lane-per-row 16-byte load touches
    // -- these launches were bound by the texture path, not by the number of load rounds), written row-major with pitch 36
    // and read back as the MFMA fragments.  Blocks that reach beyond the bulk columns (bias / extra column) or the
    // wavefront's last groups take the lane-per-row loads.
    float* const myA = stA + wave * (32 * SK_SP);
    float* const myW = stW + wave * (32 * SK_SP);
    const int rsub = lane >> 3, chunk = lane & 7;
    const float* pa[4];
    const float* pw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pa[i] = x.zin + (size_t)min(row0 + rsub + 8 * i, max(n_rows - 1, 0)) * x.zin_pitch + zoff + 4 * chunk;
        pw[i] = W + gr.woff[g] + (size_t)min(n0 + rsub + 8 * i, n_out - 1) * Kp + 4 * chunk;
    }
    auto staged = [&](int jb) { return jb + 4 <= j1 && 8 * (jb + 4) <= x.c_in; };       // wave-uniform
    float4 ga[4], gw[4];
    auto load_blk = [&](int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { ga[i] = ldg4(pa[i] + 8 * jb); gw[i] = ldg4(pw[i] + 8 * jb); }
    };
    if (j0 < j1 && staged(j0)) load_blk(j0);
    // the operand loads above are in flight while the input layer's per-channel affine is staged in LDS
    if (x.bn.stat_sum) {                                      // the input layer's BatchNorm is finalised here (one group, zoff == 0)
        const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
        for (int i = tid; i < x.c_in; i += 64 * NW) {
            float sc, sh;
            gad_bn_fin_channel(x.bn, i, writer, sc, sh);
            sv[i] = sc;
            tv[i] = sh;
        }
    } else if (x.affine) stage_affine<64 * NW>(sv, tv, x, zoff, x.c_in);
    __syncthreads();
    for (int jb = j0; jb < j1; jb += 4) {
        if (staged(jb)) {                                     // wave-uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<float4*>(myA + (rsub + 8 * i) * SK_SP + 4 * chunk) = ga[i];
                *reinterpret_cast<float4*>(myW + (rsub + 8 * i) * SK_SP + 4 * chunk) = gw[i];
            }
            if (jb + 4 < j1 && staged(jb + 4)) load_blk(jb + 4);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                XRaw raw;
                raw.a = *reinterpret_cast<const float4*>(myA + l31 * SK_SP + 8 * u + 4 * half);
                raw.s = f4zero();
                const float4 a4 = x_finish<0>(x, raw, true, 8 * (jb + u) + 4 * half, sv, tv);
                const float4 b4 = *reinterpret_cast<const float4*>(myW + l31 * SK_SP + 8 * u + 4 * half);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
            const int je = min(jb + 4, j1);
            XRaw ra[4];
            float4 rb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(jb + u, nj - 1);
                const int col = 8 * j + 4 * half;
                ra[u] = x_raw<0>(x, r, true, zoff, col, col + 4 > x.c_in, 0);
                rb[u] = ldg4(Wg + 8 * j);
            }
            if (jb + 4 < j1 && staged(jb + 4)) load_blk(jb + 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (jb + u < je) {                            // wave-uniform
                    const float4 a4 = x_finish<0>(x, ra[u], true, 8 * (jb + u) + 4 * half, sv, tv);
                    const float4 b4 = rb[u];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) part[wave * (32 * SK_SP) + v * 64 + lane] = acc[v];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < NW; ++w)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] += part[w * (32 * SK_SP) + v * 64 + lane];
    const int n = n0 + l31;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int rr = row0 + acc_row(v, half);
        const float zv = acc[v];
        const bool live = rr < n_rows;
        if (live && n < n_out) zout[(size_t)rr * zout_pitch + ooff + n] = zv;
        const float w = live ? (row_w ? row_w[rr] : 1.f) : 0.f;
        s1 = fmaf(w, zv, s1);
        s2 = fmaf(w * zv, zv, s2);
    }
    if (stat_sum) {
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (lane < 32 && n < n_out) {
            const int rep = blockIdx.y % GAD_STAT_REPLICAS;
            atomic_add_f64(stat_sum + (size_t)rep * stat_stride + ooff + n, (double)s1);
            atomic_add_f64(stat_sq + (size_t)rep * stat_stride + ooff + n, (double)s2);
        }
    }
}

static bool fwd_skinny(const gad_gemm_fwd_args& a) {
    return !g_opt.deterministic && g_opt.fwd_skinny && a.mode == 0 && !a.n_rows_dev && a.n_rows <= 1024 && a.Kp <= SK_KCAP;
}

// the streaming kernel covers: one group, no bias / extra column, Kp in {16, 64}, n_out in {64, 128}
bool fwd_streamable(const gad_gemm_fwd_args& a) {
    if (g_opt.deterministic || !g_opt.fwd_stream) return false;
    if (a.pool_key && !(a.mode == 0 && a.n_out[0] == 128)) return false;          // pooled instantiation: 64 -> 128 only
    if (a.n_groups != 1 || a.zin_off[0] != 0 || a.w_off[0] != 0 || a.out_off[0] != 0) return false;
    if (a.n_rows < 32768 || (a.n_out[0] != 64 && a.n_out[0] != 128) || (a.zout && a.zout_pitch != a.n_out[0])) return false;
    if ((long long)a.n_rows * a.n_out[0] * 4 > (1ll << 31)) return false;              // buffer-descriptor byte offsets
    if (a.mode == 0) return a.Kp == 64 && a.c_in == 64 && a.ones_col < 0 && !a.extra && (a.scale && a.shift) && a.relu;
    const bool sa1_rows = a.feat_c == 4 && (a.action ? a.act_c == 6 : a.act_c == 0);
    if (a.mode == 2)                                                             // 64-channel input recomputed from SA1's gathered rows
        return a.Kp == 64 && a.c_in == 64 && a.n_out[0] == 64 && !a.pool_key && a.ones_col < 0 && !a.extra && a.scale && a.shift && a.relu &&
               a.pre_W && (a.pre_Kp == 8 || a.pre_Kp == 16) && sa1_rows && a.feat_c + 3 + a.act_c <= a.pre_Kp;
    // SA1's gathered rows: [f (4) | dx (3)] (policy encoder, Kp 8) or [f (4) | dx (3) | action (6)] (value encoder, Kp 16)
    return (a.Kp == 16 || a.Kp == 8) && a.feat_c == 4 && (a.action ? a.act_c == 6 : a.act_c == 0) && a.feat_c + 3 + a.act_c <= a.Kp;
}

extern "C" int gad_gemm_fwd(const gad_gemm_fwd_args* a, void* stream) {
    unsigned long long* ts = gad_take_timing_slot(stream);
    const int rows_hint = gad_take_grid_rows();
    GAD_REQUIRE(a && a->W && (a->zout || a->pool_key || a->stat_sum), GAD_ERR_NULL, "gemm_fwd: null pointer");
    GAD_REQUIRE(a->n_groups >= 1 && a->n_groups <= GAD_MAX_GROUPS, GAD_ERR_SHAPE, "gemm_fwd: n_groups");
    GAD_REQUIRE(a->Kp % 8 == 0 && a->Kp >= 8, GAD_ERR_SHAPE, "gemm_fwd: Kp=%d must be a multiple of 8", a->Kp);
    if (int e = check_input(*a, "gemm_fwd")) return e;
    if (a->n_rows <= 0) return GAD_OK;
    XSrc x = make_xsrc(*a);
    Groups gr = make_groups(a->n_groups, a->zin_off, a->w_off, a->out_off, a->n_out);
    const int nmax = max_nout(gr);
    hipStream_t st = (hipStream_t)stream;
    const int rows = a->n_rows;
    PoolEpi pe;
    pe.key = reinterpret_cast<unsigned long long*>(a->pool_key); pe.row_grp = a->pool_row_grp; pe.gamma = a->pool_gamma;
    pe.C = a->n_out[0];
    if (pe.key) {
        GAD_REQUIRE(pe.row_grp && pe.gamma, GAD_ERR_NULL, "gemm_fwd: fused max-pool needs pool_row_grp and pool_gamma");
        GAD_REQUIRE(a->mode == 0 && a->n_groups == 1 && a->out_off[0] == 0 && a->n_out[0] % 64 == 0 && rows % 4 == 0,
                    GAD_ERR_SHAPE, "gemm_fwd: fused max-pool needs an ACT input, one group, n_out %% 64 == 0, rows %% 4 == 0 (got n_out=%d rows=%d)",
                    a->n_out[0], rows);
    }
    const int grid_rows = (a->n_rows_dev && rows_hint > 0 && rows_hint < rows) ? rows_hint : rows;   // gad_grid_rows_hint
    int ncol_stats = 0;                                  // deterministic mode: statistic columns this call covers (slot width)
    for (int i = 0; i < gr.n; ++i) ncol_stats = gr.ooff[i] + gr.nout[i] > ncol_stats ? gr.ooff[i] + gr.nout[i] : ncol_stats;
    if (a->in_stat_sum) {
        GAD_REQUIRE(a->mode != 1 && a->n_groups == 1 && a->zin_off[0] == 0 && a->in_stat_sq && a->in_gamma && a->in_beta && a->scale && a->shift,
                    GAD_ERR_NULL, "gemm_fwd: input-layer BatchNorm block needs an ACT input, one group, in_stat_sq, in_gamma, in_beta, scale, shift");
        const bool has_prologue = fwd_wideable(*a) || (fwd_streamable(*a) && a->mode != 1) || (!pe.key && fwd_skinny(*a));
        if (!(has_prologue && g_opt.fwd_bn_prologue)) {               // this route reads scale / shift as given: finalise first
            if (int e = gad_bn_finalize(a->in_stat_sum, a->in_stat_sq, a->in_stat_stride, a->in_gamma, a->in_beta, a->c_in, a->in_count,
                                        a->in_eps, a->in_momentum, a->in_running_mean, a->in_running_var, const_cast<float*>(a->scale),
                                        const_cast<float*>(a->shift), a->in_mean, a->in_istd, stream)) return e;
            x.bn.stat_sum = nullptr;
        }
    }
    if (!pe.key && fwd_skinny(*a)) {
        // (a NULL zout -- statistics / pooled maxima only -- is honoured by the streaming, wide-tile and 64 x 64 kernels; this one stores unguarded)
        GAD_REQUIRE(a->zout, GAD_ERR_NULL, "gemm_fwd: zout == NULL is not supported for small-M (skinny) shapes");
        GAD_LAUNCH_SKINNY(gemm_fwd_skinny_kernel, dim3(gad_cdiv(nmax, 32), gad_cdiv(rows, 32), gr.n), st, x, gr, rows, a->row_w, a->W,
                          a->Kp, a->zout, a->zout_pitch, a->stat_sum, a->stat_sq, a->stat_stride, ts);
        GAD_CHECK_LAUNCH("gemm_fwd(skinny)");
        return GAD_OK;
    }
#define LAUNCH_FWD2(WM, WN, TM, TN, XM, POOL)                                                                  \
    do {                                                                                                   \
        constexpr int BM = WM * TM * 32, BN = WN * TN * 32;                                                \
        int gx = gad_cdiv(grid_rows, BM); if (gx > GAD_GX_CAP) gx = GAD_GX_CAP;                                        \
        if (g_opt.deterministic && a->stat_sum) {                                                          \
            double* slots = det_stat_slots(gx, ncol_stats, stream);                                        \
            if (!slots) return GAD_ERR_LAUNCH;                                                             \
            hipLaunchKernelGGL((gemm_fwd_kernel<WM, WN, TM, TN, XM, POOL, true>), dim3(gx, gad_cdiv(nmax, BN), gr.n), dim3(256), \
                               0, st, x, gr, a->n_rows_dev, rows, a->row_w, a->W, a->Kp, a->zout, a->zout_pitch, \
                               slots, slots + (size_t)gx * ncol_stats, ncol_stats, pe, ts);                \
            GAD_CHECK_LAUNCH("gemm_fwd");                                                                  \
            if (int e_ = det_stat_reduce(slots, gx, ncol_stats, a->stat_sum, a->stat_sq, stream)) return e_; \
        } else                                                                                             \
            hipLaunchKernelGGL((gemm_fwd_kernel<WM, WN, TM, TN, XM, POOL>), dim3(gx, gad_cdiv(nmax, BN), gr.n), dim3(256), \
                               0, st, x, gr, a->n_rows_dev, rows, a->row_w, a->W, a->Kp, a->zout, a->zout_pitch, \
                               a->stat_sum, a->stat_sq, a->stat_stride, pe, ts);                           \
    } while (0)
#define LAUNCH_FWD(WM, WN, TM, TN) do { if (a->mode == 0) LAUNCH_FWD2(WM, WN, TM, TN, 0, false); else LAUNCH_FWD2(WM, WN, TM, TN, 1, false); } while (0)
    if (fwd_streamable(*a)) {
        const int slabs = gad_cdiv(rows, 32);
        // one 8-wavefront workgroup per CU; the gathered first layer (K <= 16: ~100 registers, latency-bound on its five dependent
        // loads per row) may run more (option "fwd_stream_l1_wgs")
        const int gcap = a->mode == 1 ? g_opt.fwd_stream_l1_wgs : g_opt.fwd_stream_wgs;
        int gx = gad_cdiv(slabs, 8); if (gx > gcap) gx = gcap;
#define LAUNCH_STREAM(KJ, TN, XM, POOL, ...)                                                               \
        hipLaunchKernelGGL((gemm_fwd_stream_kernel<KJ, TN, XM, POOL, ##__VA_ARGS__>), dim3(gx), dim3(512), 0, st, x, a->n_rows_dev, rows, \
                           a->row_w, a->W, a->zout, a->stat_sum, a->stat_sq, a->stat_stride, pe, ts)
        if (split_on(GAD_SPLIT_FWD_STREAM) && a->mode == 0) {             // split-bf16 products (the kernel splits W itself)
            if (pe.key) LAUNCH_STREAM(8, 4, 0, true, true);
            else if (a->n_out[0] == 64) LAUNCH_STREAM(8, 2, 0, false, true);
            else LAUNCH_STREAM(8, 4, 0, false, true);
        } else if (pe.key) {
            LAUNCH_STREAM(8, 4, 0, true);                                  // (fwd_streamable: ACT input, 128 outputs)
        } else {
            if (a->mode == 2) { if (a->pre_Kp == 8) LAUNCH_STREAM(8, 2, 2, false); else LAUNCH_STREAM(8, 2, 3, false); }
            else if (a->mode == 0) { if (a->n_out[0] == 64) LAUNCH_STREAM(8, 2, 0, false); else LAUNCH_STREAM(8, 4, 0, false); }
            else if (a->Kp == 8) { if (a->n_out[0] == 64) LAUNCH_STREAM(1, 2, 1, false); else LAUNCH_STREAM(1, 4, 1, false); }
            else { if (a->n_out[0] == 64) LAUNCH_STREAM(2, 2, 1, false); else LAUNCH_STREAM(2, 4, 1, false); }
        }
#undef LAUNCH_STREAM
        if (split_on(GAD_SPLIT_FWD_STREAM) && a->mode == 0) GAD_CHECK_LAUNCH("gemm_fwd(stream split)"); else GAD_CHECK_LAUNCH("gemm_fwd(stream)");
        return GAD_OK;
    }
    if (fwd_wideable(*a)) {
        int gx = gad_cdiv(grid_rows, 64); if (gx > GAD_GX_CAP) gx = GAD_GX_CAP;
        const dim3 grid(gx, a->n_out[0] / 128);
        // split-bf16 form: family bit set and the call carries the forward weight mirror of exactly the columns the K loop covers
        const bool sp = split_on(GAD_SPLIT_FWD_WIDE) && a->W_split && a->W_split_pitch == (a->mode == 1 ? a->feat_c : a->Kp) &&
                        a->W_split_plane >= a->n_out[0] * a->W_split_pitch;
#define LAUNCH_WIDE(XM, POOL, SP)                                                                                              \
        hipLaunchKernelGGL((gemm_fwd_wide_kernel<XM, POOL, SP>), grid, dim3(256), 0, st, x, a->n_rows_dev, rows, a->row_w, a->W, a->Kp, \
                           a->n_out[0], a->zout, a->zout_pitch, a->stat_sum, a->stat_sq, a->stat_stride, pe, a->W_split, a->W_split_pitch, \
                           a->W_split_plane, ts)
        if (a->mode == 1) { if (sp) LAUNCH_WIDE(1, false, true); else LAUNCH_WIDE(1, false, false); }
        else if (pe.key) { if (sp) LAUNCH_WIDE(0, true, true); else LAUNCH_WIDE(0, true, false); }
        else { if (sp) LAUNCH_WIDE(0, false, true); else LAUNCH_WIDE(0, false, false); }
#undef LAUNCH_WIDE
        if (sp) GAD_CHECK_LAUNCH("gemm_fwd(wide split)"); else GAD_CHECK_LAUNCH("gemm_fwd(wide)");
        return GAD_OK;
    }
    // 64 x 64 tiles throughout: with K <= 1024 these launches are prologue/epilogue-bound, more and smaller
    // workgroups win over the 128-wide tiles at every shape of the step (tools/diag_gemm.py)
    if (pe.key) LAUNCH_FWD2(2, 2, 1, 1, 0, true);
    else if (nmax <= 32) LAUNCH_FWD(4, 1, 1, 1); else LAUNCH_FWD(2, 2, 1, 1);
#undef LAUNCH_FWD
#undef LAUNCH_FWD2
    GAD_CHECK_LAUNCH("gemm_fwd");
    return GAD_OK;
}
