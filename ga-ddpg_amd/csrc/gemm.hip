// Layer-GEMM family for the per-point shared MLPs, the FC head and the actor/critic heads: FP32 results throughout, products either
// on v_mfma_f32_32x32x2_f32 or -- the default for the set-abstraction layers since round 5 -- as split-bf16 term products with f32
// accumulation on v_mfma_f32_32x32x16_bf16 (six term products per product: section "split-bf16 arithmetic" of gemm_common.hpp; library option "mfma_split").
//
// Reference arithmetic replaced: the 1x1 Conv2d / Linear + BatchNorm(train) + ReLU chains that
// upstream build_shared_mlp and reference core/networks.py:84-91,280-300,339-351 run through
// cuDNN/cuBLAS, plus their autograd backward.  Nothing is materialised in the (B,C,npoint,nsample)
// layout: rows are the DE-DUPLICATED (group, point) pairs (include/gaddpg.h section B), weighted by
// their multiplicity in the BatchNorm statistics, which is exactly equivalent to the reference's
// padded neighbourhoods (duplicates change neither a max-pool nor its gradient).
//
// Hardware mapping (gfx950): v_mfma_f32_32x32x2_f32 (exact f32, 64 FLOP/clk/SIMD), 4 wavefronts
// per workgroup, operands staged k-major in LDS ([k][row], pitch = tile+1 or tile+4 so both the
// transposing ds_write_b32 and the fragment ds_read_b32 are bank-conflict free), next K-tile's
// global loads issued before the current tile's MFMAs (register-staged software pipeline).
// Producers (BN affine + ReLU, neighbourhood gather, BN-backward dZ) are fused into the operand load
// and written BRANCH-FREE (clamped addresses + selects): every 16-byte load of a tile is issued
// before the first wait, instead of one s_waitcnt per predicated load.
// BatchNorm statistics: registers -> __shfl_xor -> LDS across wavefronts -> f64 device atomics
// into one of GAD_STAT_REPLICAS accumulators (blockIdx % replicas) to bound same-address contention.
//
// Map of the family (a kernel template is defined and instantiated in exactly one unit):
//   gemm_common.hpp  what the units share: operand producers, tile staging, MFMA tile, epilogue helpers, split-bf16 arithmetic,
//                    diagnostic macros, GemmOptions, declarations of the host functions that cross the units
//   gemm.hip         this file: the option block and gad_set_option, the deterministic mode's scratch and ordered reduce, the host
//                    helpers the passes share (split_on, fits_i32_bytes, check_input, coef_fallback, det_stat_slots / _reduce)
//   gemm_fwd.hip     gad_gemm_fwd: tile, wide, streaming and skinny forward kernels
//   gemm_dx.hip      gad_gemm_dx: tile, wide, action-streaming and skinny dX kernels; the deterministic mode's ordered scatter
//   gemm_dw.hip      gad_gemm_dw: tile, skinny, streaming, gather-streaming, wide and wide-split dW kernels; dw_reduce_kernel
//   gemm_bwd.hip     gad_gemm_bwd, gad_gemm_dw_reduce: the SA1 streaming backward family (streaming dX, fused dX + dW and their split
//                    form; gad_gemm_dx reaches the first through dx_stream_launch) and the fused wide backward
// Routing: every entry point picks its kernel in its own unit, from that unit's route predicates (fwd_* / dx_* / bwd_* / dw_*able) and
// the options here; gad_last_kernel names the route taken.
#include "gemm_common.hpp"
#include <mutex>
#include <string.h>

GemmOptions g_opt;

bool split_on(int family) {
    return !g_opt.deterministic && (g_opt.mfma_split == GAD_SPLIT_ALL || (g_opt.mfma_split & family) != 0);
}

// the wide-tile kernels address their row tensors through buffer descriptors with 32-bit byte offsets: a launch whose largest
// row tensor reaches 2 GiB takes the 64 x 64 tile kernels (64-bit pointer arithmetic) instead
bool fits_i32_bytes(long long rows, int pitch_a, int pitch_b, int pitch_c, int pitch_d) {
    int p = pitch_a > pitch_b ? pitch_a : pitch_b;
    p = p > pitch_c ? p : pitch_c;
    p = p > pitch_d ? p : pitch_d;
    return rows * (long long)p * 4 <= (1ll << 31);
}

// ---- deterministic mode (option "deterministic"; include/gaddpg.h) ----
// Routing: the generic tile kernels only (every family predicate of the units answers false, split-bf16 off, gad_gemm_bwd unfused); their
// float atomics are replaced by stores of each workgroup's partial into a slot of its own (block index of a grid that depends on the
// row CAPACITY only: grid-rows hints are ignored) and one ordered column reduce (ordered_reduce_kernel) that adds the slot sums, in
// slot order, into replica 0 of the statistics or into the gradient arena.  The gathered first layers store each row's input
// gradient and ordered kernels walk the rows: point-disjoint runs for dfeat, samples for daction.  No memory is allocated here.
int gad_deterministic() { return g_opt.deterministic; }

namespace {
struct DetBuf { void* stream; int kind; void* p; size_t bytes; };
std::mutex g_det_mu;
DetBuf g_det_bufs[64];
int g_det_n = 0;
}  // namespace

void* gad_det_scratch(void* stream, int kind, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_det_mu);
    DetBuf* b = nullptr;
    for (int i = 0; i < g_det_n; ++i)
        if (g_det_bufs[i].stream == stream && g_det_bufs[i].kind == kind) b = &g_det_bufs[i];
    if (!b) {
        if (g_det_n == 64) { gad_set_error("deterministic mode: more than 64 scratch buffers (streams x kinds)"); return nullptr; }
        b = &g_det_bufs[g_det_n++];
        b->stream = stream; b->kind = kind; b->p = nullptr; b->bytes = 0;
    }
    if (b->bytes >= bytes) return b->p;
    if (b->p) {                                          // earlier launches of this stream may still read it
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipFree(b->p) != hipSuccess) {
            gad_set_error("deterministic mode: releasing a scratch buffer failed");
            b->p = nullptr; b->bytes = 0;
            return nullptr;
        }
        b->p = nullptr; b->bytes = 0;
    }
    size_t want = bytes + bytes / 4;                     // headroom: a slightly larger call does not reallocate
    want = (want + 4095) & ~(size_t)4095;
    if (hipMalloc(&b->p, want) != hipSuccess) {
        (void)hipGetLastError();
        gad_set_error("deterministic mode: cannot allocate %zu bytes of scratch", want);
        b->p = nullptr;
        return nullptr;
    }
    b->bytes = want;
    return b->p;
}

// the option's release path: switching the mode off frees every scratch buffer (hipFree waits for the work that uses them)
static void det_scratch_release() {
    std::lock_guard<std::mutex> lk(g_det_mu);
    for (int i = 0; i < g_det_n; ++i)
        if (g_det_bufs[i].p) (void)hipFree(g_det_bufs[i].p);
    g_det_n = 0;
}

// the one reduce of the mode: thread = output element, slots summed in ascending order in f64, one add into out
template <typename T>
__global__ __launch_bounds__(256) void ordered_reduce_kernel(const T* __restrict__ slots, long long slot_stride, int nslots,
                                                             long long ncols, double* __restrict__ out) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    const T* p = slots + c;
    double s = 0.0;
    for (int i = 0; i < nslots; ++i) s += (double)p[(size_t)i * slot_stride];
    atomic_add_f64(out + c, s);                          // the only add into this element in the launch
}

// the same sum for few columns over many slots (statistics, sums of squares): workgroup = column, thread t sums the slots
// t, t + 256, ... in order, then a fixed pairwise tree over the 256 threads.  The order depends on nslots only.
template <typename T>
__global__ __launch_bounds__(256) void ordered_reduce_tree_kernel(const T* __restrict__ slots, long long slot_stride, int nslots,
                                                                  double* __restrict__ out) {
    __shared__ double red[256];
    const long long c = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nslots; i += 256) s += (double)slots[(size_t)i * slot_stride + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomic_add_f64(out + c, red[0]);
}

template <typename T>
static int ordered_reduce_launch(const T* slots, long long slot_stride, int nslots, long long ncols, double* out, void* stream) {
    if (ncols <= 0 || nslots <= 0) return GAD_OK;
    if (ncols <= 4096 && nslots > 256)                   // (the form is chosen by the shape alone)
        hipLaunchKernelGGL(ordered_reduce_tree_kernel<T>, dim3((unsigned)ncols), dim3(256), 0, (hipStream_t)stream, slots, slot_stride,
                           nslots, out);
    else
        hipLaunchKernelGGL(ordered_reduce_kernel<T>, dim3(gad_cdiv(ncols, 256)), dim3(256), 0, (hipStream_t)stream, slots, slot_stride,
                           nslots, ncols, out);
    GAD_CHECK_LAUNCH("ordered_reduce");
    return GAD_OK;
}
int gad_ordered_reduce(const float* slots, long long slot_stride, int nslots, long long ncols, double* out, void* stream) {
    return ordered_reduce_launch(slots, slot_stride, nslots, ncols, out, stream);
}
int gad_ordered_reduce(const double* slots, long long slot_stride, int nslots, long long ncols, double* out, void* stream) {
    return ordered_reduce_launch(slots, slot_stride, nslots, ncols, out, stream);
}

// every GEMM option: a value inside [lo, hi] is taken as given, any other becomes `fallback` (ANY_LO .. ANY_HI: every int is taken)
constexpr int ANY_LO = -2147483647 - 1, ANY_HI = 2147483647;
static const struct { const char* name; int GemmOptions::*member; int lo, hi, fallback; } k_options[] = {
    {"deterministic", &GemmOptions::deterministic, 0, 0, 1},       // normalised: 0 is taken, everything else becomes 1
    {"mfma_split", &GemmOptions::mfma_split, ANY_LO, ANY_HI, 0},
    {"fwd_stream", &GemmOptions::fwd_stream, ANY_LO, ANY_HI, 0},
    {"fwd_wide", &GemmOptions::fwd_wide, ANY_LO, ANY_HI, 0},
    {"dx_wide", &GemmOptions::dx_wide, ANY_LO, ANY_HI, 0},
    {"dw_wide", &GemmOptions::dw_wide, ANY_LO, ANY_HI, 0},
    {"bwd_fused", &GemmOptions::bwd_fused, ANY_LO, ANY_HI, 0},
    {"bwd_wide", &GemmOptions::bwd_wide, ANY_LO, ANY_HI, 0},
    {"fwd_bn_prologue", &GemmOptions::fwd_bn_prologue, ANY_LO, ANY_HI, 0},
    {"fwd_skinny", &GemmOptions::fwd_skinny, ANY_LO, ANY_HI, 0},
    {"dx_skinny", &GemmOptions::dx_skinny, ANY_LO, ANY_HI, 0},
    {"dx_stream", &GemmOptions::dx_stream, ANY_LO, ANY_HI, 0},
    {"dw_skinny", &GemmOptions::dw_skinny, ANY_LO, ANY_HI, 0},
    {"dw_stream", &GemmOptions::dw_stream, ANY_LO, ANY_HI, 0},
    {"bwd_stream_wgs", &GemmOptions::bwd_stream_wgs, 1, DW_STREAM_SPLITS, DW_STREAM_SPLITS},
    {"fwd_stream_wgs", &GemmOptions::fwd_stream_wgs, 1, 2147483647, 256},
    {"fwd_stream_l1_wgs", &GemmOptions::fwd_stream_l1_wgs, 1, 2147483647, 256},
    {"dw_wide_wgs", &GemmOptions::dw_wide_wgs, 1, 2147483647, 256},
    {"bwd_wide_slab", &GemmOptions::bwd_wide_slab, 1, 2147483647, 4},
    {"skinny_nw", &GemmOptions::skinny_nw, 4, 4, SK_NW},            // 4 is taken, everything else becomes SK_NW (8)
};

extern "C" int gad_set_option(const char* name, int value) {
    GAD_REQUIRE(name, GAD_ERR_NULL, "set_option: null name");
    for (const auto& o : k_options) {
        if (strcmp(name, o.name)) continue;
        const int v = (value >= o.lo && value <= o.hi) ? value : o.fallback;
        // (the one option with a side effect: switching the deterministic mode off frees its scratch)
        if (o.member == &GemmOptions::deterministic && !v && g_opt.deterministic) det_scratch_release();
        g_opt.*o.member = v;
        return GAD_OK;
    }
    int found = 0;
    gad_geometry_set_option(name, value, &found);                                     // library.hip: "bq_cells", ..
    if (found) return GAD_OK;
    GAD_REQUIRE(false, GAD_ERR_SHAPE, "set_option: unknown option '%s'", name);
    return GAD_OK;
}

int check_input(const gad_gemm_fwd_args& a, const char* who) {
    if (a.mode == 2) {
        GAD_REQUIRE(!g_opt.deterministic, GAD_ERR_UNSUPPORTED, "%s: mode 2 (recomputed 64-channel input) has no deterministic form "
                    "(option \"deterministic\"): store the 64-channel input instead", who);
        GAD_REQUIRE(a.src_xyz && a.row_pt && a.row_grp && a.feat && a.pre_W, GAD_ERR_NULL, "%s: recomputed input needs the gather inputs and pre_W", who);
        GAD_REQUIRE(a.act_c == 0 || a.action, GAD_ERR_NULL, "%s: action", who);
        GAD_REQUIRE(fwd_streamable(a), GAD_ERR_SHAPE, "%s: mode 2 (recomputed 64-channel input) is a streaming-kernel form: SA1 rows, "
                    "Kp = c_in = n_out = 64, rows >= 32768, pre_Kp 8 / 16, scale / shift, relu", who);
        return GAD_OK;
    }
    if (a.mode == 0) {
        GAD_REQUIRE(a.zin && a.c_in % 4 == 0 && a.c_in >= 4 && a.c_in <= VMAX && a.zin_pitch % 4 == 0, GAD_ERR_SHAPE,
                    "%s: ACT input needs 4 <= c_in <= %d, c_in and pitch multiples of 4", who, VMAX);
        for (int i = 0; i < a.n_groups; ++i)
            GAD_REQUIRE(a.zin_off[i] % 4 == 0, GAD_ERR_SHAPE, "%s: zin_off must be a multiple of 4", who);
    } else {
        GAD_REQUIRE(a.src_xyz && a.row_pt && a.row_grp && a.feat, GAD_ERR_NULL, "%s: gather inputs", who);
        GAD_REQUIRE(a.feat_c % 4 == 0 && a.feat_c >= 4, GAD_ERR_SHAPE, "%s: feat_c must be a positive multiple of 4", who);
        GAD_REQUIRE(a.act_c == 0 || a.action, GAD_ERR_NULL, "%s: action", who);
    }
    return GAD_OK;
}

// A route whose kernels read P / Q / S per lane (no cooperative prologue) cannot form the BatchNorm-backward coefficients
// itself: gad_bn_bwd_coef runs first, into the caller's coefP / Q / S scratch, and the block is dropped.
int coef_fallback(gad_dz_src& dz, void* stream) {
    if (!dz.bn_dbeta) return GAD_OK;
    GAD_REQUIRE(dz.coefP && dz.coefQ && dz.coefS && dz.scale && dz.bn_dgamma && dz.bn_mean && dz.bn_istd, GAD_ERR_NULL,
                "BatchNorm-backward block on a route without a prologue needs coefP / Q / S scratch");
    if (int e = gad_bn_bwd_coef(dz.bn_dbeta, dz.bn_dgamma, dz.bn_stride, dz.scale, dz.bn_mean, dz.bn_istd, dz.c, dz.bn_count,
                                const_cast<float*>(dz.coefP), const_cast<float*>(dz.coefQ), const_cast<float*>(dz.coefS), dz.gacc_gamma,
                                dz.gacc_beta, stream)) return e;
    dz.bn_dbeta = nullptr; dz.bn_dgamma = nullptr; dz.gacc_gamma = nullptr; dz.gacc_beta = nullptr;
    return GAD_OK;
}

// deterministic mode: zeroed slot planes (sum, square) of gx rows x ncol doubles for one statistics launch (blocks that return early
// leave zeros), and their ordered sums into replica 0
double* det_stat_slots(int gx, int ncol, void* stream) {
    const size_t n = 2 * (size_t)gx * ncol;
    double* p = static_cast<double*>(gad_det_scratch(stream, GAD_DET_SLOTS, n * sizeof(double)));
    if (p && hipMemsetAsync(p, 0, n * sizeof(double), (hipStream_t)stream) != hipSuccess) {
        gad_set_error("deterministic mode: clearing the statistic slots failed");
        return nullptr;
    }
    return p;
}
int det_stat_reduce(const double* slots, int gx, int ncol, double* sum, double* sq, void* stream) {
    if (int e = gad_ordered_reduce(slots, ncol, gx, ncol, sum, stream)) return e;
    return gad_ordered_reduce(slots + (size_t)gx * ncol, ncol, gx, ncol, sq, stream);
}
