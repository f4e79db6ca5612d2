// dX pass of the layer-GEMM family (overview and map of the units: gemm.hip): the tile, wide, action-streaming and skinny kernels,
// the deterministic mode's ordered scatter, the route predicates and gad_gemm_dx.  (The SA1 streaming dX kernels: gemm_bwd.hip.)
#include "gemm_common.hpp"

// ------------------------------------------------------------------------------------------------
// backward wrt the layer input:  gout[r][k] = sum_n dZ[r][n] * W[n][k]
// ------------------------------------------------------------------------------------------------
// DET (deterministic mode): e.dbeta / e.dgamma are slot planes of e.stat_stride doubles per block (as in gemm_fwd_kernel)
template <int WM, int WN, int TM, int TN, bool VEC, int VM, bool DET = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_dx_kernel(DzSrc d, Groups gr, const int32_t* __restrict__ n_rows_dev,
                                                       int n_rows_static, const float* __restrict__ W, int Kp,
                                                       DxEpi e, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int PA = PitchT<BM>::v, PB = PitchD<BN>::v;
    constexpr int UA = BM * 8 / 256, UB = BN * 8 / 256;
    constexpr int OFFB = (KT * PA + 3) & ~3;
    constexpr int TILE = OFFB + KT * PB;
    constexpr int SM = TILE + 3 * BM + (VEC ? 5 * VM : 4);
    static_assert(TILE >= 2 * WM * BN, "reduction scratch must fit in the tile LDS");
    __shared__ __attribute__((aligned(16))) float smem[SM];
    float* As = smem;
    float* Bs = smem + OFFB;
    int32_t* ptS = reinterpret_cast<int32_t*>(smem + TILE);
    int32_t* grS = ptS + BM;
    float* wS = reinterpret_cast<float*>(grS + BM);
    float* vec = wS + BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = blockIdx.z;
    const int doff = gr.aoff[g], n_out = gr.nout[g], goff = gr.ooff[g];
    const float* Wg = W + gr.woff[g];
    const int k0out = blockIdx.y * BN;
    if (k0out >= e.k_valid) return;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if ((int)(blockIdx.x * BM) >= n_rows) return;
    const int nk = gad_cdiv_dev(n_out, KT);
    if (VEC) stage_dz_vecs<VM>(vec, d, doff, n_out);
    const bool need_grp = e.mode == 1 || d.gmode != 0;

    float cb[TN], cg[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) { cb[t] = 0.f; cg[t] = 0.f; }

    for (int row0 = blockIdx.x * BM; row0 < n_rows; row0 += gridDim.x * BM) {
        f32x16 acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
        if (tid < BM) {
            const int r = row0 + tid;
            const bool ok = r < n_rows;
            wS[tid] = (ok && d.row_w) ? d.row_w[r] : 1.f;
            if (e.mode == 1) ptS[tid] = ok ? e.row_pt[r] : 0;
            if (need_grp) grS[tid] = ok ? (e.mode == 1 ? e.row_grp[r] : d.row_grp[r]) : 0;
        }
        __syncthreads();

        DzRaw ra[UA];
        float4 rb[UB];
        auto load_tile = [&](int kt) {
            const int nb = kt * KT;
#pragma unroll
            for (int it = 0; it < UA; ++it) {
                int i, kk; unit_T<BM>(it * 256 + tid, i, kk);
                const int r = row0 + i;
                ra[it] = dz_raw<VEC>(d, r, r < n_rows, doff, nb + kk, n_out, need_grp ? grS[i] : 0);
            }
#pragma unroll
            for (int it = 0; it < UB; ++it) {
                int kk, j; unit_D<BN>(it * 256 + tid, kk, j);
                const int n = nb + kk, k = k0out + j;
                const bool ok = n < n_out && k < Kp;
                rb[it] = ldg4(Wg + (size_t)(ok ? n : 0) * Kp + (ok ? k : 0));
            }
        };
        auto store_tile = [&](int kt) {
            const int nb = kt * KT;
#pragma unroll
            for (int it = 0; it < UA; ++it) {
                int i, kk; unit_T<BM>(it * 256 + tid, i, kk);
                const int r = row0 + i;
                store_T<BM>(As, i, kk, dz_finish<VEC, VM>(d, ra[it], r, r < n_rows, nb + kk, n_out, wS[i], vec));
            }
#pragma unroll
            for (int it = 0; it < UB; ++it) {
                int kk, j; unit_D<BN>(it * 256 + tid, kk, j);
                const bool ok = (nb + kk) < n_out && (k0out + j) < Kp;
                store_D<BN>(Bs, kk, j, f4sel(ok, rb[it], f4zero()));
            }
        };
        load_tile(0);
        for (int kt = 0; kt < nk; ++kt) {
            store_tile(kt);
            __syncthreads();
            if (kt + 1 < nk) load_tile(kt + 1);
            mfma_ktile<TM, TN, PA, PB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
            __syncthreads();
        }
        const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int k = k0out + wn * TN * 32 + tn * 32 + l31;
            const bool kok = k < e.k_valid;
            float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
            const bool stats = e.dbeta != nullptr && kok;
            if (stats) { sc = e.ps[goff + k]; sh = e.pt[goff + k]; mu = e.pm[goff + k]; is = e.pi[goff + k]; }
            float sb = 0.f, sg = 0.f;
            int run_smp = -1;
            double run_sum = 0.0;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int il = wm * TM * 32 + tm * 32 + acc_row(v, half);
                    const int r = row0 + il;
                    if (r >= n_rows || !kok) continue;
                    const float gv = acc[tm][tn][v];
                    if (e.mode == 0) {
                        float outv = gv;
                        if (stats) {
                            const float zp = e.zprev[(size_t)r * e.zprev_pitch + goff + k];
                            if (fmaf(zp, sc, sh) > 0.f) { sb += gv; sg = fmaf(gv, (zp - mu) * is, sg); }
                            else if (e.store_masked) outv = 0.f;
                        }
                        e.gout[(size_t)r * e.gout_pitch + goff + k] = outv;
                    } else {
                        // gather-layer columns: [feat (feat_c) | xyz (3) | action (act_c)]
                        if (k < e.feat_c) {
                            if (e.dfeat) atomic_add_f32(e.dfeat + (size_t)ptS[il] * e.feat_c + k, gv);
                        } else if (k >= e.feat_c + 3 && k < e.feat_c + 3 + e.act_c) {
                            // per-sample action gradient: ~875 rows of a sample add into the same 6 addresses.  The rows a
                            // lane holds are consecutive runs of a tile, almost always of ONE sample: accumulate the run
                            // in a register and issue one f64 atomic per run instead of one per row
                            if (e.daction) {
                                const int smp = grS[il] / e.gps;
                                if (smp != run_smp) {
                                    if (run_smp >= 0) atomic_add_f64(e.daction + (size_t)run_smp * e.act_c + (k - e.feat_c - 3), run_sum);
                                    run_smp = smp; run_sum = 0.0;
                                }
                                run_sum += (double)gv;
                            }
                        }
                    }
                }
            if (run_smp >= 0) atomic_add_f64(e.daction + (size_t)run_smp * e.act_c + (k - e.feat_c - 3), run_sum);
            cb[tn] += sb; cg[tn] += sg;
        }
        __syncthreads();
    }
    if (e.dbeta) {
        const int rep = DET ? blockIdx.x : blockIdx.x % GAD_STAT_REPLICAS;
        block_column_atomics<WM, WN, TN, DET>(smem, cb, cg, lane, wm, wn, k0out, e.k_valid,
                                              e.dbeta + (size_t)rep * e.stat_stride + goff,
                                              e.dgamma + (size_t)rep * e.stat_stride + goff);
    }
}

// ------------------------------------------------------------------------------------------------
// wide-tile dX for the MID-SIZE layers (the backward twin of gemm_fwd_wide_kernel): a workgroup owns 64 rows x 128 input
// channels of gout, a wavefront 32 x 64.  A operand: dZ[r][n] = P*dY - w*(Q + S*z) formed once per staged element from
// 16-byte loads of z and dY (or of the pooled arg-max / gradient pair; the ReLU mask is already in dY: premasked), stored
// row-major ([row][32 + 4]: one ds_read_b128 per four MFMA steps); B operand: W[n][k] kept AS STORED in LDS ([n][128 + 4], one
// ds_write_b128 per staged float4), its fragments are conflict-free ds_read_b32 across k of row n = 8j+4h+i.  (Round 3 wrote
// the W tile TRANSPOSED -- four ds_write_b32 per float4, 6 - 8 % bank-conflict cycles, 10 - 14 % LDS waits -- to read it back
// with ds_read_b128: round 4 measured the stored layout 18 % faster, 20 - 37 us -> 16 - 30 us per launch, +2.3 % steps/s.)
// Epilogue: dY of the previous layer masked by its ReLU (store_masked) + that layer's BatchNorm-backward sums.
// ------------------------------------------------------------------------------------------------
// SC = 1: scatter epilogue of the gathered first layers (SA2 / SA3: dX columns = the feature channels of the row's point):
// float atomics into dfeat[row_pt[r]][k], nothing stored per row, no BatchNorm in front
// SP: split-bf16 products (namespace spw): dZ is split while it is staged, the B side is the layer's TRANSPOSED weight mirror
// (rows = input channels k, the reduction index n contiguous: wsp, pitch = n_out).
template <int GM, int SC, bool SP = false>
__global__ __launch_bounds__(256, 2) void gemm_dx_wide_kernel(DzSrc d, const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                              const float* __restrict__ W, int Kp, int n_out, DxEpi e,
                                                              const uint16_t* __restrict__ wsp, int wsp_plane,
                                                              unsigned long long* __restrict__ ts) {
    KTimer kt_(ts);
    constexpr int BM = 64, BN = 128, P = KT + 4, PB = BN + 4, STAGE = SP ? spw::STAGE / 4 : BM * P + KT * PB, VM = 512;
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + 3 * VM + BM];
    __shared__ int32_t ptS[BM];                          // SC: the tile rows' points
    float* vP = smem + 2 * STAGE;                        // P | Q | S of this layer's channels
    float* wS = vP + 3 * VM;
    int32_t* grS = reinterpret_cast<int32_t*>(wS);       // (pooled source: the rows' groups share the slot with the weights: see below)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int k0out = blockIdx.y * BN;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if ((int)(blockIdx.x * BM) >= n_rows) return;
    const int nk = n_out / KT;
    // every global operand through a buffer descriptor: one 32-bit byte offset per lane and tile + a wave-uniform scalar offset
    // per access instead of a 64-bit pointer multiply-add per load / store (on this part every VALU instruction is MFMA issue
    // time: the epilogue's 64 address computations per tile were a third of the vector instructions of the N = 128 layers)
    const int gpitch = GM == 0 ? d.g_pitch : d.c;
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.z), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t gr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GM == 0 ? d.G : d.dout), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(GM == 0 ? d.row_grp : d.argmax), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, GAD_BUF_MAX, 0x00020000);
    // previous layer's raw output / the gradient this launch writes: bounded by the live rows (reads past them give 0,
    // stores past them are dropped)
    const int zp_pitch4 = SC ? 0 : e.zprev_pitch * 4, go_pitch4 = SC ? 0 : e.gout_pitch * 4;
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(SC ? W : e.zprev), 0, SC ? 0 : gad_nbytes(n_rows, zp_pitch4), 0x00020000);
    const __amdgpu_buffer_rsrc_t or_ = __builtin_amdgcn_make_buffer_rsrc(SC ? const_cast<float*>(W) : e.gout, 0, SC ? 0 : gad_nbytes(n_rows, go_pitch4), 0x00020000);
    const int c4 = (tid & 7) * 4, ur = tid >> 3;         // A staging: 16-byte chunk of the K-tile, row (ur, ur + 32)
    const int bk4 = (tid & 31) * 4, bn = tid >> 5;       // B staging: W rows bn, +8, +16, +24 of the K-tile, k chunk bk4
    int vw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vw[u] = ((bn + 8 * u) * Kp + k0out + bk4) * 4;
    // SP: rows k0out + (tid >> 2) + 64 u of the transposed mirror, 16-byte chunk tid & 3 of a K-tile's 32 output channels
    const __amdgpu_buffer_rsrc_t ws_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(SP ? wsp : reinterpret_cast<const uint16_t*>(W)), 0, GAD_BUF_MAX, 0x00020000);
    int vbs[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) vbs[u] = ((k0out + (tid >> 2) + 64 * u) * n_out + (tid & 3) * 8) * 2;
    unsigned char* const smem_b = reinterpret_cast<unsigned char*>(smem);
    const int sp_fo = ((half ^ ((l31 >> 2) & 3)) << 4);
    for (int i = tid; i < n_out; i += 256) {
        float Pc, Qc, Sc;
        dz_coef(d, i, Pc, Qc, Sc, first_workgroup());
        vP[i] = Pc; vP[VM + i] = Qc; vP[2 * VM + i] = Sc;
    }
    (void)grS;
    // previous layer's BatchNorm vectors of this lane's two output columns
    float ps[2] = {0.f, 0.f}, pt[2] = {0.f, 0.f}, pm[2] = {0.f, 0.f}, pi[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k = k0out + wn * 64 + t * 32 + l31;
        if (!SC) { ps[t] = e.ps[k]; pt[t] = e.pt[k]; pm[t] = e.pm[k]; pi[t] = e.pi[k]; }
    }
    float cb[2] = {0.f, 0.f}, cg[2] = {0.f, 0.f};
    for (int row0 = blockIdx.x * BM; row0 < n_rows; row0 += gridDim.x * BM) {
        f32x16 acc[2];
        f32x16 an[2];                                    // SP: the negated accumulators (odd k16-steps)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[t][v] = 0.f; if (SP) an[t][v] = 0.f; }
        // this thread's two staged rows (clamped past the live count: their dZ is zeroed through the weight / validity)
        int vz[2], vg[2];
        float wrow[2];
        bool live[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = row0 + ur + 32 * u;
            live[u] = r < n_rows;
            const int rr = live[u] ? r : max(n_rows - 1, 0);
            wrow[u] = d.row_w ? d.row_w[rr] : 1.f;
            vz[u] = (rr * d.z_pitch + c4) * 4;
            vg[u] = ((GM == 1 ? d.row_grp[rr] : rr) * gpitch + c4) * 4;
        }
        float4 rz[2], rg[2], rb[SP ? 1 : 4];
        gad_u32x4 ra[2];
        spw::BRegs rbs;
        auto load_regs = [&](int kt) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                rz[u] = buf_ld4(zr, vz[u], kt * (KT * 4));
                rg[u] = buf_ld4(gr_, vg[u], kt * (KT * 4));
                if (GM == 1) ra[u] = __builtin_amdgcn_raw_buffer_load_b128(ar, vg[u], kt * (KT * 4), 0);
            }
            if (SP) { spw::load_b(rbs, ws_, vbs, wsp_plane * 2, kt); return; }
#pragma unroll
            for (int u = 0; u < (SP ? 1 : 4); ++u) rb[u] = buf_ld4(wr, vw[u], kt * (KT * 4) * Kp);
        };
        auto write_lds = [&](int kt) {
            float* As = smem + (kt & 1) * STAGE;
            float* Bs = As + BM * P;
            const int nb = kt * KT + c4;
            const float4 P4 = *reinterpret_cast<const float4*>(vP + nb), Q4 = *reinterpret_cast<const float4*>(vP + VM + nb);
            const float4 S4 = *reinterpret_cast<const float4*>(vP + 2 * VM + nb);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float4 g = rg[u];
                const float4 z = rz[u];
                if (GM == 1) {
                    const unsigned r = row0 + ur + 32 * u;   // the true row (a clamped row never matches an arg-max)
                    g.x = ra[u].x == r ? g.x : 0.f; g.y = ra[u].y == r ? g.y : 0.f;
                    g.z = ra[u].z == r ? g.z : 0.f; g.w = ra[u].w == r ? g.w : 0.f;
                }
                const float w = wrow[u];
                float4 v;
                v.x = P4.x * g.x - w * fmaf(S4.x, z.x, Q4.x); v.y = P4.y * g.y - w * fmaf(S4.y, z.y, Q4.y);
                v.z = P4.z * g.z - w * fmaf(S4.z, z.z, Q4.z); v.w = P4.w * g.w - w * fmaf(S4.w, z.w, Q4.w);
                if (!live[u]) v = f4zero();
                if (SP) spw::store_a4(smem_b + (kt & 1) * spw::STAGE, ur + 32 * u, tid, v, (ur & 1) ? 0x80000000u : 0u);
                else *reinterpret_cast<float4*>(As + (ur + 32 * u) * P + c4) = v;
            }
            if (SP) { spw::store_b(smem_b + (kt & 1) * spw::STAGE, rbs, tid); return; }
#pragma unroll
            for (int u = 0; u < (SP ? 1 : 4); ++u)           // W[n][k..k+3] as stored: Bs[n][k], one ds_write_b128 (no transposing stores)
                *reinterpret_cast<float4*>(Bs + (bn + 8 * u) * PB + bk4) = rb[u];
        };
        load_regs(0);
        __syncthreads();                                 // vP visible; the previous row tile's LDS reads are done
        if (SC && tid < BM) ptS[tid] = e.row_pt[min(row0 + tid, max(n_rows - 1, 0))];     // (read after the K loop's barriers)
        write_lds(0);
        if (nk > 1) load_regs(1);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            if (SP) {
                spw::ktile(smem_b + (kt & 1) * spw::STAGE, (wm * 32 + l31) * 64, (wn * 64 + l31) * 64, sp_fo, acc, an);
                if (kt + 1 < nk) write_lds(kt + 1);
                if (kt + 2 < nk) load_regs(kt + 2);
                __syncthreads();
                continue;
            }
            const float* As = smem + (kt & 1) * STAGE + (wm * 32 + l31) * P + 4 * half;
            // B fragments: row n = 8 j + 4 h + i of the stored tile, this lane's column -- conflict-free ds_read_b32 across k
            const float* Bs = smem + (kt & 1) * STAGE + BM * P + (4 * half) * PB + wn * 64 + l31;
            float4 a4 = *reinterpret_cast<const float4*>(As);
            float4 b0 = make_float4(Bs[0], Bs[PB], Bs[2 * PB], Bs[3 * PB]);
            float4 b1 = make_float4(Bs[32], Bs[PB + 32], Bs[2 * PB + 32], Bs[3 * PB + 32]);
#pragma unroll
            for (int j = 0; j < KT / 8; ++j) {
                float4 an = a4, bn0 = b0, bn1 = b1;
                if (j + 1 < KT / 8) {
                    an = *reinterpret_cast<const float4*>(As + 8 * (j + 1));
                    const float* bq = Bs + 8 * (j + 1) * PB;
                    bn0 = make_float4(bq[0], bq[PB], bq[2 * PB], bq[3 * PB]);
                    bn1 = make_float4(bq[32], bq[PB + 32], bq[2 * PB + 32], bq[3 * PB + 32]);
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
            if (kt + 1 < nk) write_lds(kt + 1);
            if (kt + 2 < nk) load_regs(kt + 2);
            __syncthreads();
        }
        if (SP) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][v] = (v & 1) ? an[t][v] - acc[t][v] : acc[t][v] - an[t][v];   // (odd rows entered negated)
        }
        // epilogue: dY of the previous layer (ReLU-masked) + its BatchNorm-backward sums; all z_prev loads first
        if (SC) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k = k0out + wn * 64 + t * 32 + l31;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int il = wm * 32 + acc_row(v, half);
                    if (row0 + il < n_rows) atomic_add_f32(e.dfeat + (size_t)ptS[il] * e.feat_c + k, acc[t][v]);
                }
            }
            continue;
        }
        // (a row past the live count: z_prev reads 0 through the bounded descriptor, its accumulator row is exactly 0 -- its dZ
        // was zeroed -- and the store is dropped)
        const int rb0 = row0 + wm * 32;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int kcol = k0out + wn * 64 + t * 32 + l31;
            const int vzp = (4 * half * e.zprev_pitch + kcol) * 4, vgo = (4 * half * e.gout_pitch + kcol) * 4;
            float zp[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) zp[v] = buf_ld(pr, vzp, (rb0 + (v & 3) + 8 * (v >> 2)) * zp_pitch4);
            const float npm = -pm[t] * pi[t];
            float sb = 0.f, sg = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float ga = fmaf(zp[v], ps[t], pt[t]) > 0.f ? acc[t][v] : 0.f;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ga), or_, vgo, (rb0 + (v & 3) + 8 * (v >> 2)) * go_pitch4, 0);
                sb += ga;
                sg = fmaf(ga, fmaf(zp[v], pi[t], npm), sg);
            }
            cb[t] += sb; cg[t] += sg;
        }
    }
    if (SC) return;
    const int rep = blockIdx.x % GAD_STAT_REPLICAS;
    block_column_atomics<2, 2, 2>(smem, cb, cg, lane, wm, wn, k0out, e.k_valid, e.dbeta + (size_t)rep * e.stat_stride,
                                  e.dgamma + (size_t)rep * e.stat_stride);
}

// ------------------------------------------------------------------------------------------------
// dX of the value encoder's SA1 first layer, of which only the ACTION columns are wanted (the gradient of Q(s, pi(s)) with
// respect to pi: reference core/ddpg.py:160-177): daction[sample][a] = sum over the sample's rows of dZ[r][:] . W[:][c0 + a].
// A 64-channel dot product per row and action component: HBM-bound (z and dY: 512 B per row), no MFMA.  16 lanes per row
// (one coalesced 256-byte row per quarter wavefront), a contiguous row range per wavefront, so the rows of a sample (~830,
// consecutive) are summed in registers and leave through six f64 atomics per sample and wavefront.  (The 64 x 64 tile
// kernel spent 63 us here forming all 16 input columns with MFMAs at 4 % of their peak.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dx_action_stream_kernel(DzSrc d, const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                               const float* __restrict__ W, int Kp, int c0, DxEpi e,
                                                               unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    const int n_waves = gridDim.x * 4;
    const int gw = blockIdx.x * 4 + (tid >> 6);
    int chunk = (n_rows + n_waves - 1) / n_waves;
    chunk = (chunk + 3) & ~3;
    const int r0 = gw * chunk, r1 = min(n_rows, r0 + chunk);
    if (r0 >= r1) return;
    const int sub = lane >> 4, c4 = (lane & 15) * 4;
    float4 P, Q, S;
    dz_coef(d, c4 + 0, P.x, Q.x, S.x); dz_coef(d, c4 + 1, P.y, Q.y, S.y);
    dz_coef(d, c4 + 2, P.z, Q.z, S.z); dz_coef(d, c4 + 3, P.w, Q.w, S.w);
    float4 wa[6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
        wa[a] = make_float4(W[(size_t)(c4 + 0) * Kp + c0 + a], W[(size_t)(c4 + 1) * Kp + c0 + a], W[(size_t)(c4 + 2) * Kp + c0 + a],
                            W[(size_t)(c4 + 3) * Kp + c0 + a]);
    double run[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cur = -1;                                                    // the open sample (wave-uniform)
    auto flush = [&]() {
        if (cur >= 0 && lane == 0)
#pragma unroll
            for (int a = 0; a < 6; ++a) atomic_add_f64(e.daction + (size_t)cur * 6 + a, run[a]);
#pragma unroll
        for (int a = 0; a < 6; ++a) run[a] = 0.0;
    };
    for (int rb = r0; rb < r1; rb += 4) {
        const int r = rb + sub;
        const bool live = r < r1;
        const int rr = live ? r : r1 - 1;
        const float4 z = ldg4(d.z + (size_t)rr * d.z_pitch + c4);
        const float4 g = ldg4(d.G + (size_t)rr * d.g_pitch + c4);
        const float w = d.row_w ? d.row_w[rr] : 1.f;
        const int smp = e.row_grp[rr] / e.gps;
        float4 dz;
        dz.x = P.x * g.x - w * fmaf(S.x, z.x, Q.x); dz.y = P.y * g.y - w * fmaf(S.y, z.y, Q.y);
        dz.z = P.z * g.z - w * fmaf(S.z, z.z, Q.z); dz.w = P.w * g.w - w * fmaf(S.w, z.w, Q.w);
        float p[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            p[a] = fmaf(dz.x, wa[a].x, fmaf(dz.y, wa[a].y, fmaf(dz.z, wa[a].z, dz.w * wa[a].w)));
            p[a] = live ? p[a] : 0.f;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) p[a] += __shfl_xor(p[a], m, 16);        // the row's 16 lanes
        }
        const int s0 = __builtin_amdgcn_readlane(smp, 0), s1 = __builtin_amdgcn_readlane(smp, 16);
        const int s2 = __builtin_amdgcn_readlane(smp, 32), s3 = __builtin_amdgcn_readlane(smp, 48);
        if (s0 == s1 && s1 == s2 && s2 == s3) {                      // wave-uniform: the four rows are of one sample
            if (s0 != cur) { flush(); cur = s0; }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                float t = p[a] + __shfl_xor(p[a], 16, 64);
                t += __shfl_xor(t, 32, 64);
                run[a] += (double)t;
            }
        } else {                                                     // a sample boundary inside the four rows: row by row
            flush();
            cur = -1;
            if ((lane & 15) == 0 && live)
#pragma unroll
                for (int a = 0; a < 6; ++a) atomic_add_f64(e.daction + (size_t)smp * 6 + a, (double)p[a]);
        }
    }
    flush();
}

// the action-gradient layer: scatter epilogue that wants nothing but daction, G source, 64 channels, 6 action components
static bool dx_action_streamable(const gad_gemm_dx_args& a, bool vec) {
    if (g_opt.deterministic || !g_opt.dx_stream || !vec || a.n_groups != 1 || a.dz_off[0] != 0 || a.w_off[0] != 0) return false;
    if (a.epilogue != 1 || a.dfeat || !a.daction || a.act_c != 6 || !a.row_grp || a.n_rows < 32768 || a.n_out[0] != 64) return false;
    const gad_dz_src& d = a.dz;
    return d.gmode == 0 && d.G && d.z && d.z_pitch % 4 == 0 && d.g_pitch % 4 == 0 && d.premasked && d.coefP && d.coefQ && d.coefS &&
           a.feat_c + 3 + a.act_c <= a.Kp;
}

static bool dx_wideable(const gad_gemm_dx_args& a, bool vec) {
    if (g_opt.deterministic || !g_opt.dx_wide || !vec || a.n_groups != 1 || a.dz_off[0] != 0 || a.w_off[0] != 0 || a.gout_off[0] != 0) return false;
    if (a.n_rows < 2048 || a.k_valid % 128 != 0 || a.k_valid > a.Kp) return false;
    if (a.n_out[0] % 32 != 0 || a.n_out[0] < 32 || a.n_out[0] > 512) return false;
    if (a.epilogue == 1) {                               // scatter into the points' feature gradients (SA2 / SA3 first layers)
        if (g_opt.dx_wide == 2 || !a.dfeat || a.daction || !a.row_pt || a.k_valid != a.feat_c || a.prev_dbeta) return false;
    } else if (!a.prev_dbeta || !a.store_masked || !(a.zprev && a.prev_scale && a.prev_shift && a.prev_mean && a.prev_istd && a.prev_dgamma)) return false;
    const gad_dz_src& d = a.dz;
    if (!d.z || d.z_pitch % 4 != 0 || !d.relu || !d.premasked || !(d.coefP && d.coefQ && d.coefS)) return false;
    if (!fits_i32_bytes(a.n_rows, d.z_pitch, d.gmode == 0 ? d.g_pitch : d.c, a.epilogue == 0 ? a.gout_pitch : 0, a.epilogue == 0 ? a.zprev_pitch : 0)) return false;
    return d.gmode == 0 ? (d.g_pitch % 4 == 0 && d.G) : (d.c % 4 == 0);
}

// skinny dX for the small-M layers (same idea as gemm_fwd_skinny_kernel): one 32x32 tile of gout per workgroup, the 8
// wavefronts split the reduction over the layer's output channels n.  A operand = dZ[r][8j+4h..+3] (16-byte loads of
// z and G, BatchNorm-backward applied in registers), B operand = W[8j+4h+i][k0+lane%32]: four 4-byte loads per group
// of 8 channels, each a fully coalesced 128-byte row segment -- no transposed weight copy needed.
template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_dx_skinny_kernel(DzSrc d, Groups gr, int n_rows,
                                                                    const float* __restrict__ W, int Kp, DxEpi e, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    __shared__ __attribute__((aligned(16))) float stZ[NW * 32 * SK_SP], stG[NW * 32 * SK_SP];
    float* const part = stZ;                                  // partial tiles reuse the wavefront's own operand stage
    __shared__ __attribute__((aligned(16))) float vec[5 * VMAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int g = blockIdx.z;
    const int doff = gr.aoff[g], n_out = gr.nout[g], goff = gr.ooff[g];
    const int k0 = blockIdx.x * 32, row0 = blockIdx.y * 32;      // (x = column tile: see gemm_fwd_skinny_kernel)
    for (int i = tid; i < n_out; i += 64 * NW) {
        vec[i] = d.scale ? d.scale[doff + i] : 1.f;
        vec[VMAX + i] = d.shift ? d.shift[doff + i] : 0.f;
        float P, Q, S;
        dz_coef(d, doff + i, P, Q, S, first_workgroup());
        vec[2 * VMAX + i] = P; vec[3 * VMAX + i] = Q; vec[4 * VMAX + i] = S;
    }
    __syncthreads();
    const int r = min(row0 + l31, max(n_rows - 1, 0));                // clamped: extra rows are not stored
    const int k = min(k0 + l31, Kp - 1);
    const float* Wg = W + gr.woff[g] + k;
    const float wrow = d.row_w ? d.row_w[r] : 1.f;
    const int nj = (n_out + 7) >> 3;
    const int per = (nj + NW - 1) / NW;
    const int j0 = wave * per, j1 = min(nj, j0 + per);

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    // z and dY blocks of four channel groups go through a wavefront-private LDS stage, loaded coalesced (see
    // gemm_fwd_skinny_kernel); the W fragments are coalesced as they are.  Two blocks per loop trip: static register sets.
    float* const myZ = stZ + wave * (32 * SK_SP);
    float* const myG = stG + wave * (32 * SK_SP);
    const int rsub = lane >> 3, chunk = lane & 7;
    const float* pz[4];
    const float* pg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t rr = (size_t)min(row0 + rsub + 8 * i, max(n_rows - 1, 0));
        pz[i] = d.z ? d.z + rr * d.z_pitch + doff + 4 * chunk : nullptr;
        pg[i] = d.G + rr * d.g_pitch + doff + 4 * chunk;
    }
    auto staged = [&](int jb) { return d.z != nullptr && jb + 4 <= j1 && 8 * (jb + 4) <= n_out; };     // wave-uniform
    float4 gz[4], gg[4], rb[2][4];
    auto load_blk = [&](int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { gz[i] = ldg4(pz[i] + 8 * jb); gg[i] = ldg4(pg[i] + 8 * jb); }
    };
    auto load_w = [&](int jb, auto bufc) {
        constexpr int B = decltype(bufc)::value;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int n = 8 * min(jb + u, nj - 1) + 4 * half;
            const int nc = n < n_out ? n : 0;                 // clamped; dz_finish zeroes n >= n_out
            const float* wp = Wg + (size_t)nc * Kp;
            rb[B][u] = make_float4(wp[0], wp[Kp], wp[2 * (size_t)Kp], wp[3 * (size_t)Kp]);
        }
    };
    auto block = [&](int jb, auto bufc) {
        constexpr int B = decltype(bufc)::value;
        const bool more = jb + 4 < j1;
        float4 rz[4], rg[4];
        const bool st = staged(jb);
        if (st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<float4*>(myZ + (rsub + 8 * i) * SK_SP + 4 * chunk) = gz[i];
                *reinterpret_cast<float4*>(myG + (rsub + 8 * i) * SK_SP + 4 * chunk) = gg[i];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = 8 * min(jb + u, nj - 1) + 4 * half;
                const int nc = n < n_out ? n : 0;
                rz[u] = d.z ? ldg4(d.z + (size_t)r * d.z_pitch + doff + nc) : f4zero();
                rg[u] = ldg4(d.G + (size_t)r * d.g_pitch + doff + nc);
            }
        }
        if (more) {
            if (staged(jb + 4)) load_blk(jb + 4);
            load_w(jb + 4, std::integral_constant<int, B ^ 1>{});
        }
        if (st) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                rz[u] = *reinterpret_cast<const float4*>(myZ + l31 * SK_SP + 8 * u + 4 * half);
                rg[u] = *reinterpret_cast<const float4*>(myG + l31 * SK_SP + 8 * u + 4 * half);
            }
        }
        const int je = min(jb + 4, j1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (jb + u < je) {                                // wave-uniform
                DzRaw raw;
                raw.z = rz[u]; raw.g = rg[u]; raw.a = make_int4(0, 0, 0, 0);
                const float4 a4 = dz_finish<true>(d, raw, r, true, 8 * (jb + u) + 4 * half, n_out, wrow, vec);
                const float4 b4 = rb[B][u];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
            }
        }
        if (st) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    };
    if (j0 < j1) {
        if (staged(j0)) load_blk(j0);
        load_w(j0, std::integral_constant<int, 0>{});
    }
    for (int jb = j0; jb < j1; jb += 8) {
        block(jb, std::integral_constant<int, 0>{});
        if (jb + 4 < j1) block(jb + 4, std::integral_constant<int, 1>{});
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) part[wave * (32 * SK_SP) + v * 64 + lane] = acc[v];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < NW; ++w)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] += part[w * (32 * SK_SP) + v * 64 + lane];
    const int kk = k0 + l31;
    const bool kok = kk < e.k_valid;
    const bool stats = e.dbeta != nullptr && kok;
    float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
    if (stats) { sc = e.ps[goff + kk]; sh = e.pt[goff + kk]; mu = e.pm[goff + kk]; is = e.pi[goff + kk]; }
    float sb = 0.f, sg = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int rr = row0 + acc_row(v, half);
        if (rr >= n_rows || !kok) continue;
        const float gv = acc[v];
        float outv = gv;
        if (stats) {
            const float zp = e.zprev[(size_t)rr * e.zprev_pitch + goff + kk];
            if (fmaf(zp, sc, sh) > 0.f) { sb += gv; sg = fmaf(gv, (zp - mu) * is, sg); }
            else if (e.store_masked) outv = 0.f;
        }
        e.gout[(size_t)rr * e.gout_pitch + goff + kk] = outv;
    }
    if (e.dbeta) {
        sb += __shfl_xor(sb, 32, 64);
        sg += __shfl_xor(sg, 32, 64);
        if (lane < 32 && kok) {
            const int rep = blockIdx.y % GAD_STAT_REPLICAS;
            atomic_add_f64(e.dbeta + (size_t)rep * e.stat_stride + goff + kk, (double)sb);
            atomic_add_f64(e.dgamma + (size_t)rep * e.stat_stride + goff + kk, (double)sg);
        }
    }
}

// deterministic mode, gathered first layer.  rowbuf = the rows' input gradients [row][pitch] (feature columns, 3 coordinate
// columns, action columns), as gemm_dx_kernel stored them; rows are ordered by group (include/gaddpg.h section B).
__device__ __forceinline__ int rows_lower_bound(const int32_t* __restrict__ row_grp, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row_grp[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Feature columns: the rows are cut into RUNS that share no point, found from the data alone (no reliance on grp_per_sample): a
// cut goes before group g when every point the rows before it reference is below every point the rows from g on reference
// (prefix max < suffix min).  One workgroup per run, thread = column, the run's rows walked in ascending order: each point's
// contributions all lie in one run, so every dfeat element is written by one thread, in row order.  With the ball query's rows
// (a sample's rows reference only its own points, samples' points ascending) a run is at most one sample.
// (1) per-group point bounds: gmin / gmax (empty group: INT_MAX / -1); G > gcap marks the whole call as one run
__global__ __launch_bounds__(256) void scatter_group_bounds_kernel(const int32_t* __restrict__ row_pt, const int32_t* __restrict__ row_grp,
                                                                   const int32_t* __restrict__ n_rows_dev, int n_rows_static, int gcap,
                                                                   int32_t* __restrict__ gmin, int32_t* __restrict__ gmax) {
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if (n_rows <= 0) return;
    const int G = min(row_grp[n_rows - 1] + 1, gcap);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int r0 = rows_lower_bound(row_grp, n_rows, g), r1 = rows_lower_bound(row_grp, n_rows, g + 1);
    int lo = INT_MAX, hi = -1;
    for (int r = r0; r < r1; ++r) { const int p = row_pt[r]; lo = min(lo, p); hi = max(hi, p); }
    gmin[g] = lo;
    gmax[g] = hi;
}
// (2) one workgroup: head[g] = 1 where a run starts (prefix max of gmax before g < suffix min of gmin from g on)
__global__ __launch_bounds__(256) void scatter_run_heads_kernel(const int32_t* __restrict__ row_grp, const int32_t* __restrict__ n_rows_dev,
                                                                int n_rows_static, int gcap, const int32_t* __restrict__ gmin,
                                                                const int32_t* __restrict__ gmax, int32_t* __restrict__ head) {
    __shared__ int32_t lmax[256], lmin[256];
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if (n_rows <= 0) return;
    const int Gall = row_grp[n_rows - 1] + 1;
    const int G = min(Gall, gcap);
    const int t = threadIdx.x, chunk = (G + 255) / 256;
    const int g0 = min(G, t * chunk), g1 = min(G, g0 + chunk);
    int mx = -1, mn = INT_MAX;
    for (int g = g0; g < g1; ++g) { mx = max(mx, gmax[g]); mn = min(mn, gmin[g]); }
    lmax[t] = mx; lmin[t] = mn;
    __syncthreads();
    if (t == 0) {                                        // exclusive prefix max / suffix min over the 256 chunks, in place
        int run = -1;
        for (int i = 0; i < 256; ++i) { const int v = lmax[i]; lmax[i] = run; run = max(run, v); }
        run = INT_MAX;
        for (int i = 255; i >= 0; --i) { const int v = lmin[i]; lmin[i] = run; run = min(run, v); }
    }
    __syncthreads();
    int sm = lmin[t];
    for (int g = g1 - 1; g >= g0; --g) { sm = min(sm, gmin[g]); head[g] = sm; }      // suffix min from g on
    int pm = lmax[t];
    for (int g = g0; g < g1; ++g) {
        const int suf = head[g];
        head[g] = (g == 0 || pm < suf) && Gall <= gcap ? 1 : 0;
        pm = max(pm, gmax[g]);
    }
    if (Gall > gcap && t == 0) head[0] = 1;              // (more groups than the bounds arrays hold: one run)
}
// (3) the runs
__global__ __launch_bounds__(256) void scatter_runs_kernel(const float* __restrict__ rowbuf, int pitch, const int32_t* __restrict__ row_pt,
                                                           const int32_t* __restrict__ row_grp, const int32_t* __restrict__ n_rows_dev,
                                                           int n_rows_static, int gcap, const int32_t* __restrict__ head, int feat_c,
                                                           float* dfeat) {
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if (n_rows <= 0) return;
    const int Gall = row_grp[n_rows - 1] + 1;
    const int G = min(Gall, gcap);
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        if (!head[g]) continue;
        int ge = g + 1;
        while (ge < G && !head[ge]) ++ge;
        const int r0 = rows_lower_bound(row_grp, n_rows, g);
        const int r1 = ge < G ? rows_lower_bound(row_grp, n_rows, ge) : n_rows;
        for (int c = threadIdx.x; c < feat_c; c += 256)
            for (int r = r0; r < r1; ++r) {
                float* p = dfeat + (size_t)row_pt[r] * feat_c + c;
                *p = *p + rowbuf[(size_t)r * pitch + c];
            }
    }
}

// Action columns (per-sample sums: the sample of a row is row_grp / grp_per_sample, as in the default kernels): one workgroup per
// sample, thread = column, the sample's rows summed in ascending order in f64 and added once into daction.
__global__ __launch_bounds__(256) void gather_action_ordered_kernel(const float* __restrict__ rowbuf, int pitch,
                                                                    const int32_t* __restrict__ row_grp, const int32_t* __restrict__ n_rows_dev,
                                                                    int n_rows_static, int gps, int act_off, int act_c, double* daction) {
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    if (n_rows <= 0) return;
    const int n_smp = row_grp[n_rows - 1] / gps + 1;
    for (int s = blockIdx.x; s < n_smp; s += gridDim.x) {
        const int r0 = rows_lower_bound(row_grp, n_rows, s * gps), r1 = rows_lower_bound(row_grp, n_rows, (s + 1) * gps);
        for (int j = threadIdx.x; j < act_c; j += 256) {
            double acc = 0.0;
            for (int r = r0; r < r1; ++r) acc += (double)rowbuf[(size_t)r * pitch + act_off + j];
            daction[(size_t)s * act_c + j] += acc;
        }
    }
}

// the 64 x 64 tile dX launch of the deterministic mode: statistics through slots + ordered reduce; the gathered first layer's scatter
// as row-buffer stores (the same kernel's plain-store epilogue) + the ordered scatter kernels above
template <int WM, int WN, int TM, int TN, bool V>
static int det_dx_launch(const gad_gemm_dx_args* a, const DzSrc& d, Groups gr, DxEpi e, int gx, int nmax_dx, unsigned long long* ts,
                         void* stream) {
    constexpr int BN = WN * TN * 32;
    hipStream_t st = (hipStream_t)stream;
    const int rows = a->n_rows, kv = a->k_valid;
    const dim3 grid(gx, gad_cdiv(kv, BN), gr.n);
    double* slots = nullptr;
    int ncol = 0;
    if (e.mode == 1) {
        GAD_REQUIRE(gr.n == 1 && !e.dbeta, GAD_ERR_UNSUPPORTED, "gemm_dx: the deterministic scatter epilogue takes one group and no "
                    "previous-layer statistics");
        GAD_REQUIRE(kv >= (a->daction && a->act_c > 0 ? a->feat_c + 3 + a->act_c : a->feat_c), GAD_ERR_SHAPE,
                    "gemm_dx: k_valid=%d does not cover the scattered columns", kv);
        float* rowbuf = static_cast<float*>(gad_det_scratch(stream, GAD_DET_ROWS, (size_t)rows * kv * sizeof(float)));
        if (!rowbuf) return GAD_ERR_LAUNCH;
        e.mode = 0; e.gout = rowbuf; e.gout_pitch = kv; e.store_masked = 0;
        gr.ooff[0] = 0;
    } else if (e.dbeta) {
        for (int i = 0; i < gr.n; ++i) ncol = gr.ooff[i] + kv > ncol ? gr.ooff[i] + kv : ncol;
        slots = det_stat_slots(gx, ncol, stream);
        if (!slots) return GAD_ERR_LAUNCH;
        e.dbeta = slots; e.dgamma = slots + (size_t)gx * ncol; e.stat_stride = ncol;
    }
    if (slots) {
        if (nmax_dx <= 512) hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, 512, true>), grid, dim3(256), 0, st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);
        else                hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, VMAX, true>), grid, dim3(256), 0, st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);
    } else {
        if (nmax_dx <= 512) hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, 512>), grid, dim3(256), 0, st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);
        else                hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, VMAX>), grid, dim3(256), 0, st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);
    }
    GAD_CHECK_LAUNCH("gemm_dx");
    if (slots) return det_stat_reduce(slots, gx, ncol, a->prev_dbeta, a->prev_dgamma, stream);
    if (a->epilogue == 1 && a->dfeat) {
        const int gcap = rows;                           // (a group has at least one row: at most `rows` groups)
        int32_t* b = static_cast<int32_t*>(gad_det_scratch(stream, GAD_DET_RUNS, 3 * (size_t)gcap * sizeof(int32_t)));
        if (!b) return GAD_ERR_LAUNCH;
        int32_t *gmin = b, *gmax = b + gcap, *head = b + 2 * (size_t)gcap;
        hipLaunchKernelGGL(scatter_group_bounds_kernel, dim3(gad_cdiv(gcap, 256)), dim3(256), 0, st, a->row_pt, a->row_grp, a->n_rows_dev,
                           rows, gcap, gmin, gmax);
        hipLaunchKernelGGL(scatter_run_heads_kernel, dim3(1), dim3(256), 0, st, a->row_grp, a->n_rows_dev, rows, gcap, gmin, gmax, head);
        hipLaunchKernelGGL(scatter_runs_kernel, dim3(1024), dim3(256), 0, st, e.gout, kv, a->row_pt, a->row_grp, a->n_rows_dev, rows, gcap,
                           head, a->feat_c, a->dfeat);
        GAD_CHECK_LAUNCH("scatter_runs");
    }
    if (a->epilogue == 1 && a->daction && a->act_c > 0) {
        hipLaunchKernelGGL(gather_action_ordered_kernel, dim3(1024), dim3(256), 0, st, e.gout, kv, a->row_grp, a->n_rows_dev, rows, e.gps,
                           a->feat_c + 3, a->act_c, a->daction);
        GAD_CHECK_LAUNCH("gather_action_ordered");
    }
    return GAD_OK;
}

extern "C" int gad_gemm_dx(const gad_gemm_dx_args* a, void* stream) {
    unsigned long long* ts = gad_take_timing_slot(stream);
    const int rows_hint = gad_take_grid_rows();
    GAD_REQUIRE(a && a->W, GAD_ERR_NULL, "gemm_dx: null pointer");
    GAD_REQUIRE(a->n_groups >= 1 && a->n_groups <= GAD_MAX_GROUPS, GAD_ERR_SHAPE, "gemm_dx: n_groups");
    GAD_REQUIRE(a->Kp % 8 == 0, GAD_ERR_SHAPE, "gemm_dx: Kp must be a multiple of 8");
    GAD_REQUIRE(a->epilogue == 1 || a->gout, GAD_ERR_NULL, "gemm_dx: gout");
    // every group STORES its own gout columns: no kernel adds the groups of one launch into shared columns
    GAD_REQUIRE(a->accumulate == 0 || a->n_groups == 1, GAD_ERR_UNSUPPORTED, "gemm_dx: accumulate=%d with %d groups is not implemented "
                "(groups store, they do not add: concatenate the groups into one, or give each its own gout_off)", a->accumulate, a->n_groups);
    GAD_REQUIRE(a->dz.gmode == 0 ? a->dz.G != nullptr : (a->dz.argmax && a->dz.dout && a->dz.row_grp), GAD_ERR_NULL,
                "gemm_dx: gradient source");
    if (a->n_rows <= 0) return GAD_OK;
    DzSrc d = make_dzsrc(a->dz);
    Groups gr = make_groups(a->n_groups, a->dz_off, a->w_off, a->gout_off, a->n_out);
    DxEpi e = make_dxepi(*a);
    GAD_REQUIRE(e.mode == 0 || (e.row_pt && e.row_grp), GAD_ERR_NULL, "gemm_dx: scatter epilogue needs row maps");
    GAD_REQUIRE(!e.dbeta || (e.zprev && e.ps && e.pt && e.pm && e.pi && e.dgamma), GAD_ERR_NULL, "gemm_dx: prev BN stats inputs");
    hipStream_t st = (hipStream_t)stream;
    const int rows = a->n_rows, kv = a->k_valid;
    const int grid_rows = (a->n_rows_dev && rows_hint > 0 && rows_hint < rows) ? rows_hint : rows;   // gad_grid_rows_hint
    const bool vec = dz_vectorizable(a->dz, a->dz_off, a->n_out, a->n_groups);
    if (dx_streamable(*a, vec)) return dx_stream_launch(a, d, e, ts, stream);
    if (dx_action_streamable(*a, vec)) {
        if (a->dz.bn_dbeta) {                            // per-lane coefficients: formed by gad_bn_bwd_coef first
            gad_dz_src dz2 = a->dz;
            if (int e2 = coef_fallback(dz2, stream)) return e2;
            d = make_dzsrc(dz2);
        }
        hipLaunchKernelGGL(dx_action_stream_kernel, dim3(1024), dim3(256), 0, st, d, a->n_rows_dev, rows, a->W, a->Kp, a->feat_c + 3, e, ts);
        GAD_CHECK_LAUNCH("gemm_dx(action stream)");
        return GAD_OK;
    }
    if (dx_wideable(*a, vec)) {
        int gx = gad_cdiv(grid_rows, 64); if (gx > GAD_GX_CAP) gx = GAD_GX_CAP;
        const dim3 grid(gx, kv / 128);
        // split-bf16 form: family bit set, the call carries the transposed weight mirror, the reduction (n_out) is whole K-tiles
        const bool sp = split_on(GAD_SPLIT_DX_WIDE) && a->W_split_t && a->W_split_t_pitch == a->n_out[0] && a->n_out[0] % 32 == 0 &&
                        a->W_split_t_plane >= kv * a->n_out[0];
#define LAUNCH_DXW(GM, SC, SP)                                                                                                 \
        hipLaunchKernelGGL((gemm_dx_wide_kernel<GM, SC, SP>), grid, dim3(256), 0, st, d, a->n_rows_dev, rows, a->W, a->Kp, a->n_out[0], e, \
                           a->W_split_t, a->W_split_t_plane, ts)
        if (a->epilogue == 1 && a->dz.gmode == 0) { if (sp) LAUNCH_DXW(0, 1, true); else LAUNCH_DXW(0, 1, false); }
        else if (a->dz.gmode == 0) { if (sp) LAUNCH_DXW(0, 0, true); else LAUNCH_DXW(0, 0, false); }
        else { if (sp) LAUNCH_DXW(1, 0, true); else LAUNCH_DXW(1, 0, false); }
#undef LAUNCH_DXW
        if (sp) GAD_CHECK_LAUNCH("gemm_dx(wide split)"); else GAD_CHECK_LAUNCH("gemm_dx(wide)");
        return GAD_OK;
    }
    int nmax_dx = 0;
    for (int i = 0; i < a->n_groups; ++i) nmax_dx = a->n_out[i] > nmax_dx ? a->n_out[i] : nmax_dx;
    if (!g_opt.deterministic && g_opt.dx_skinny && vec && e.mode == 0 && a->dz.gmode == 0 && !a->n_rows_dev && rows <= 1024 &&
        nmax_dx <= VMAX) {
        GAD_LAUNCH_SKINNY(gemm_dx_skinny_kernel, dim3(gad_cdiv(kv, 32), gad_cdiv(rows, 32), gr.n), st, d, gr, rows, a->W, a->Kp, e, ts);
        GAD_CHECK_LAUNCH("gemm_dx(skinny)");
        return GAD_OK;
    }
#define LAUNCH_DX2(WM, WN, TM, TN, V)                                                                    \
    do {                                                                                                 \
        constexpr int BM = WM * TM * 32, BN = WN * TN * 32;                                              \
        int gx = gad_cdiv(grid_rows, BM); if (gx > GAD_GX_CAP) gx = GAD_GX_CAP;                                      \
        if (g_opt.deterministic) {                                                                       \
            if (int e_ = det_dx_launch<WM, WN, TM, TN, V>(a, d, gr, e, gx, nmax_dx, ts, stream)) return e_; \
            return GAD_OK;                                                                               \
        }                                                                                                \
        if (nmax_dx <= 512)                                                                              \
            hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, 512>), dim3(gx, gad_cdiv(kv, BN), gr.n), dim3(256), 0, \
                               st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);                          \
        else                                                                                             \
            hipLaunchKernelGGL((gemm_dx_kernel<WM, WN, TM, TN, V, VMAX>), dim3(gx, gad_cdiv(kv, BN), gr.n), dim3(256), 0, \
                               st, d, gr, a->n_rows_dev, rows, a->W, a->Kp, e, ts);                          \
    } while (0)
#define LAUNCH_DX(WM, WN, TM, TN) do { if (vec) LAUNCH_DX2(WM, WN, TM, TN, true); else LAUNCH_DX2(WM, WN, TM, TN, false); } while (0)
    // 64 x 64 tiles (or 128 x 32 for narrow outputs): measured best on the whole step, also for the 2e5-row SA1
    // layers (128 x 64: -3.7 % steps/s, 128 x 128: -16 %)
    if (kv <= 32) LAUNCH_DX(4, 1, 1, 1); else LAUNCH_DX(2, 2, 1, 1);
#undef LAUNCH_DX
#undef LAUNCH_DX2
    GAD_CHECK_LAUNCH("gemm_dx");
    return GAD_OK;
}
