// Observation geometry (gaddpg.h section A, "depth frame -> point state"): what the reference does per control step on the host
// in numpy -- core/utils.py:454-491 (backproject_camera_target[_realworld]), :308-314 (se3_transform_pc), env/panda_scene.py:
// 442-450, 698-714, 1178-1206 (_get_observation, update_curr_acc_points, process_pointcloud) -- as three device operators:
//
//   gad_backproject_depth    depth image + mask -> the kept pixels' points, compacted in ascending pixel order (numpy's X[:, mask])
//   gad_cloud_gather_affine  dst[j] = A . src[sel[j]] + t            (the subsample + se3_transform_pc of the accumulated cloud)
//   gad_point_state_pack     (lead points | A . src[sel[j]] + t) -> channel-major (4, n_lead + n) state, the inverse of gad_prep_points
//
// All three are bound by memory traffic (5 B read and at most 16 B written per pixel; 12 B read and 12 / 16 B written per point),
// so the code below is about access shape only: 16-byte depth loads, one pass per byte, stores contiguous along the point axis.
//
// Compaction scheme of gad_backproject_depth.  An image is cut into tiles of 1024 consecutive pixels of its flattened form, one
// 256-thread workgroup per tile, four consecutive pixels per lane (lane-major: ascending lane = ascending pixel).  Three launches,
// ordered by the stream alone -- no workgroup waits for another inside a launch and no atomic places a point:
//   (1) count    every tile's number of kept pixels -> workspace[b * ntiles + t]
//   (2) scan     one workgroup per image turns its tile counts into exclusive offsets in place and writes count[b]
//   (3) scatter  re-evaluates the keep predicate, ranks the kept pixels inside the tile and stores point tile_offset + rank
// The rank inside a wavefront comes from four ballots (one per pixel slot of the lanes) and mbcnt -- kept pixels of lower lanes --
// plus the lane's own lower slots; the four wavefront totals of a tile go through LDS.  The result is the stable compaction: it
// does not depend on scheduling.
#include "common.hpp"

namespace {

constexpr int BP_T = 256;                 // threads of a tile's workgroup
constexpr int BP_TILE = 4 * BP_T;         // pixels of a tile
constexpr int OBS_MAX_HW = 4096;          // H, W limit: pixel coordinates stay exact in float32 with room to spare

// kept pixels in lanes below this one
__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__device__ __forceinline__ float depth_metres(float v, float) { return v; }
__device__ __forceinline__ float depth_metres(uint16_t v, float div) { return (float)v / div; }     // IEEE division, as astype(float32) / div

// the lane's four pixels p0 .. p0 + 3 of one image (`depth` / `mask` point at the image): depths in d[], bit j of the result set
// iff pixel p0 + j exists, d != 0 (a NaN is kept) and its mask byte is 0.  One 16-byte (float) / 8-byte (uint16) depth load and
// one 4-byte mask load where the four pixels exist and the address is aligned, element loads otherwise (image tails; images whose
// start is not aligned because H * W is no multiple of 4).
template <typename D>
__device__ __forceinline__ unsigned load_four(const D* __restrict__ depth, const uint8_t* __restrict__ mask, int p0, int HW,
                                              float div, float d[4]) {
    unsigned exist = 0, masked = 0;
    D raw[4] = {D(0), D(0), D(0), D(0)};
    if (p0 + 4 <= HW) {
        exist = 15u;
        const D* dp = depth + p0;
        if ((reinterpret_cast<uintptr_t>(dp) & (4 * sizeof(D) - 1)) == 0) {
            struct alignas(4 * sizeof(D)) quad { D v[4]; };
            const quad q = *reinterpret_cast<const quad*>(dp);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = q.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = dp[j];
        }
        if (mask) {
            const uint8_t* mp = mask + p0;
            if ((reinterpret_cast<uintptr_t>(mp) & 3) == 0) {
                const uint32_t m = *reinterpret_cast<const uint32_t*>(mp);
#pragma unroll
                for (int j = 0; j < 4; ++j) masked |= ((m >> (8 * j)) & 255u) ? (1u << j) : 0u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) masked |= mp[j] ? (1u << j) : 0u;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p0 + j < HW) {
                exist |= 1u << j;
                raw[j] = depth[p0 + j];
                if (mask && mask[p0 + j]) masked |= 1u << j;
            }
        }
    }
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[j] = depth_metres(raw[j], div);
        if (d[j] != 0.f) keep |= 1u << j;          // (true for a NaN)
    }
    return keep & exist & ~masked;
}

template <typename D>
__global__ __launch_bounds__(BP_T) void backproject_count_kernel(const D* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                 int HW, int ntiles, float div, int32_t* __restrict__ tile_cnt) {
    __shared__ int wtot[BP_T / 64];
    const int b = blockIdx.x / ntiles, t = blockIdx.x - b * ntiles;
    const size_t img = (size_t)b * HW;
    float d[4];
    const unsigned keep = load_four(depth + img, mask ? mask + img : nullptr, t * BP_TILE + 4 * (int)threadIdx.x, HW, div, d);
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) total += __popcll(__ballot((keep >> j) & 1u));
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// exclusive scan of one image's tile counts, in place, 256 tiles per pass; count[b] = the image's kept pixels
__global__ __launch_bounds__(BP_T) void backproject_scan_kernel(int32_t* __restrict__ tile_cnt, int ntiles, int32_t* __restrict__ count) {
    __shared__ int wtot[BP_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* c = tile_cnt + (size_t)blockIdx.x * ntiles;
    int run = 0;                                           // kept pixels of the passes before this one (uniform)
    for (int base = 0; base < ntiles; base += BP_T) {
        const int i = base + tid;
        const int v = i < ntiles ? c[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BP_T / 64; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (i < ntiles) c[i] = run + before + (inc - v);
        run += total;
        __syncthreads();                                   // wtot is rewritten by the next pass
    }
    if (tid == 0) count[blockIdx.x] = run;
}

// P_k = d * ((M[k][0] * x + M[k][1] * y) + M[k][2]) + t_k, every operation individually rounded (A = rows [M[k][0..2], t_k])
__device__ __forceinline__ void backproject_point(const float* A, float x, float y, float d, float out[3]) {
    // hipcc contracts a*b+c into an FMA by default: only operators written under this pragma stay individually rounded
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mx = A[4 * k + 0] * x, my = A[4 * k + 1] * y;
        const float r = (mx + my) + A[4 * k + 2];
        const float dr = d * r;
        out[k] = dr + A[4 * k + 3];
    }
}

template <typename D>
__global__ __launch_bounds__(BP_T) void backproject_scatter_kernel(const D* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                   const float* __restrict__ A, int HW, int W, int ntiles, float div,
                                                                   const int32_t* __restrict__ tile_off, float* __restrict__ xyz,
                                                                   int32_t* __restrict__ pix) {
    __shared__ int wtot[BP_T / 64];
    const int b = blockIdx.x / ntiles, t = blockIdx.x - b * ntiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)b * HW;
    const int p0 = t * BP_TILE + 4 * (int)threadIdx.x;
    float d[4];
    const unsigned keep = load_four(depth + img, mask ? mask + img : nullptr, p0, HW, div, d);
    int below = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long bal = __ballot((keep >> j) & 1u);
        below += lanes_below(bal);
        total += __popcll(bal);
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    int rank = tile_off[blockIdx.x] + below;
#pragma unroll
    for (int w = 0; w < BP_T / 64; ++w)
        if (w < wave) rank += wtot[w];
    if (!keep) return;
    float Ab[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Ab[i] = A[(size_t)b * 12 + i];
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (((keep >> j) & 1u) && rank < HW) {             // (rank < HW always holds while the inputs do not change between the launches)
            float P[3];
            backproject_point(Ab, (float)x, (float)y, d[j], P);
            float* o = xyz + (img + rank) * 3;
            o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
            if (pix) pix[img + rank] = p0 + j;
            ++rank;
        }
        if (++x == W) { x = 0; ++y; }
    }
}

int backproject_check(const char* who, int B, int H, int W, int* ntiles) {
    GAD_REQUIRE(B >= 0, GAD_ERR_SHAPE, "%s: unsupported batch B=%d", who, B);
    GAD_REQUIRE(H >= 1 && H <= OBS_MAX_HW && W >= 1 && W <= OBS_MAX_HW, GAD_ERR_SHAPE, "%s: image of H=%d x W=%d outside 1..%d", who, H,
                W, OBS_MAX_HW);
    GAD_REQUIRE((long long)B * H * W < (1ll << 31), GAD_ERR_SHAPE, "%s: B * H * W = %d * %d * %d is beyond 2^31", who, B, H, W);
    *ntiles = gad_cdiv((long long)H * W, BP_TILE);
    // (hipLaunchKernelGGL takes the grid in threads: workgroups x 256 has to stay below 2^32)
    GAD_REQUIRE((long long)B * *ntiles < (1ll << 23), GAD_ERR_SHAPE, "%s: a grid of B * tiles = %d * %d workgroups overflows", who, B,
                *ntiles);
    return GAD_OK;
}

template <typename D>
void backproject_launch(const void* depth, float div, const uint8_t* mask, const float* A, int B, int HW, int W, int ntiles, float* xyz,
                        int32_t* count, int32_t* pix, int32_t* tiles, hipStream_t st) {
    const D* dp = static_cast<const D*>(depth);
    hipLaunchKernelGGL(backproject_count_kernel<D>, dim3(B * ntiles), dim3(BP_T), 0, st, dp, mask, HW, ntiles, div, tiles);
    hipLaunchKernelGGL(backproject_scan_kernel, dim3(B), dim3(BP_T), 0, st, tiles, ntiles, count);
    hipLaunchKernelGGL(backproject_scatter_kernel<D>, dim3(B * ntiles), dim3(BP_T), 0, st, dp, mask, A, HW, W, ntiles, div, tiles, xyz,
                       pix);
}

// ((M[k][0] * x + M[k][1] * y) + M[k][2] * z) + t_k, every operation individually rounded; A == NULL copies the point
__device__ __forceinline__ void affine_point(const float* __restrict__ A, float x, float y, float z, float out[3]) {
#pragma clang fp contract(off)
    if (!A) {
        out[0] = x; out[1] = y; out[2] = z;
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mx = A[4 * k + 0] * x, my = A[4 * k + 1] * y, mz = A[4 * k + 2] * z;
        out[k] = ((mx + my) + mz) + A[4 * k + 3];
    }
}

__global__ __launch_bounds__(256) void cloud_gather_affine_kernel(const float* __restrict__ src, long long src_stride,
                                                                  const int32_t* __restrict__ sel, const float* __restrict__ A, int n,
                                                                  long long total, float* __restrict__ dst, long long dst_stride) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int b = (int)(q / n), j = (int)(q - (long long)b * n);
    const float* s = src + b * src_stride + 3 * (size_t)(sel ? sel[q] : j);
    float P[3];
    affine_point(A ? A + (size_t)b * 12 : nullptr, s[0], s[1], s[2], P);
    float* o = dst + b * dst_stride + 3 * (size_t)j;
    o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
}

// one thread per state column: the four channel rows are each written contiguously along the point axis
__global__ __launch_bounds__(256) void point_state_pack_kernel(const float* __restrict__ src, long long src_stride,
                                                               const int32_t* __restrict__ sel, const float* __restrict__ A,
                                                               const float* __restrict__ lead, int n_lead, float lead_flag, int n,
                                                               long long total, float* __restrict__ state) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int NP = n_lead + n;
    const int b = (int)(q / NP), col = (int)(q - (long long)b * NP);
    float P[3], flag;
    if (col < n_lead) {
        P[0] = lead[3 * col + 0]; P[1] = lead[3 * col + 1]; P[2] = lead[3 * col + 2];
        flag = lead_flag;
    } else {
        const int j = col - n_lead;
        const float* s = src + b * src_stride + 3 * (size_t)(sel ? sel[(size_t)b * n + j] : j);
        affine_point(A ? A + (size_t)b * 12 : nullptr, s[0], s[1], s[2], P);
        flag = 0.f;
    }
    float* o = state + (size_t)b * 4 * NP + col;
    o[0] = P[0]; o[(size_t)NP] = P[1]; o[(size_t)2 * NP] = P[2]; o[(size_t)3 * NP] = flag;
}

}        // namespace

extern "C" long long gad_backproject_depth_workspace_bytes(int B, int H, int W) {
    int ntiles = 0;
    const int rc = backproject_check("backproject_depth_workspace_bytes", B, H, W, &ntiles);
    if (rc != GAD_OK) return rc;
    return ((long long)B * ntiles * 4 + 255) & ~255ll;         // one i32 per tile: its count, then its offset
}

extern "C" int gad_backproject_depth(const void* depth, int depth_u16, float depth_div, const uint8_t* mask, const float* A, int B, int H,
                                     int W, float* xyz, int32_t* count, int32_t* pix, void* workspace, void* stream) {
    int ntiles = 0;
    const int rc = backproject_check("backproject_depth", B, H, W, &ntiles);
    if (rc != GAD_OK) return rc;
    GAD_REQUIRE(depth_u16 == 0 || depth_u16 == 1, GAD_ERR_SHAPE, "backproject_depth: depth_u16=%d is neither 0 (float32) nor 1 (uint16)",
                depth_u16);
    GAD_REQUIRE(!depth_u16 || (depth_div > 0.f && depth_div <= 3.0e38f), GAD_ERR_SHAPE,
                "backproject_depth: a uint16 depth needs a finite divisor > 0, got %g", (double)depth_div);
    if (B == 0) return GAD_OK;
    GAD_REQUIRE(depth && A && xyz && count, GAD_ERR_NULL, "backproject_depth: null pointer (depth / A / xyz / count)");
    GAD_REQUIRE(workspace, GAD_ERR_NULL, "backproject_depth: null pointer (workspace)");
    GAD_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, GAD_ERR_SHAPE, "backproject_depth: the workspace must be 8-byte aligned");
    GAD_REQUIRE((reinterpret_cast<size_t>(depth) & (depth_u16 ? 1 : 3)) == 0, GAD_ERR_SHAPE,
                "backproject_depth: the depth image is not aligned to its element size");
    int32_t* tiles = static_cast<int32_t*>(workspace);
    if (depth_u16)
        backproject_launch<uint16_t>(depth, depth_div, mask, A, B, H * W, W, ntiles, xyz, count, pix, tiles, (hipStream_t)stream);
    else
        backproject_launch<float>(depth, 1.f, mask, A, B, H * W, W, ntiles, xyz, count, pix, tiles, (hipStream_t)stream);
    GAD_CHECK_LAUNCH("backproject_depth");
    return GAD_OK;
}

static int cloud_args_check(const char* who, const float* src, int src_stride, int B, int n) {
    GAD_REQUIRE(B >= 0 && n >= 0 && src_stride >= 0, GAD_ERR_SHAPE, "%s: unsupported shape B=%d n=%d src_stride=%d", who, B, n, src_stride);
    GAD_REQUIRE(src || (long long)B * n == 0, GAD_ERR_NULL, "%s: null pointer (src)", who);
    return GAD_OK;
}

extern "C" int gad_cloud_gather_affine(const float* src, int src_stride, const int32_t* sel, const float* A, int B, int n, float* dst,
                                       int dst_stride, void* stream) {
    const int rc = cloud_args_check("cloud_gather_affine", src, src_stride, B, n);
    if (rc != GAD_OK) return rc;
    GAD_REQUIRE(dst_stride >= 0, GAD_ERR_SHAPE, "cloud_gather_affine: negative dst_stride=%d", dst_stride);
    const long long total = (long long)B * n;
    GAD_REQUIRE(total < (1ll << 31), GAD_ERR_SHAPE, "cloud_gather_affine: B * n = %d * %d is beyond 2^31", B, n);
    if (total == 0) return GAD_OK;
    GAD_REQUIRE(dst, GAD_ERR_NULL, "cloud_gather_affine: null pointer (dst)");
    hipLaunchKernelGGL(cloud_gather_affine_kernel, dim3(gad_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, (long long)src_stride,
                       sel, A, n, total, dst, (long long)dst_stride);
    GAD_CHECK_LAUNCH("cloud_gather_affine");
    return GAD_OK;
}

extern "C" int gad_point_state_pack(const float* src, int src_stride, const int32_t* sel, const float* A, const float* lead, int n_lead,
                                    float lead_flag, int B, int n, float* state, void* stream) {
    const int rc = cloud_args_check("point_state_pack", src, src_stride, B, n);
    if (rc != GAD_OK) return rc;
    GAD_REQUIRE(n_lead >= 0, GAD_ERR_SHAPE, "point_state_pack: negative n_lead=%d", n_lead);
    GAD_REQUIRE(lead || n_lead == 0, GAD_ERR_NULL, "point_state_pack: null pointer (lead) with n_lead=%d", n_lead);
    const long long total = (long long)B * ((long long)n_lead + n);
    GAD_REQUIRE(total < (1ll << 31), GAD_ERR_SHAPE, "point_state_pack: B * (n_lead + n) = %d * (%d + %d) is beyond 2^31", B, n_lead, n);
    if (total == 0) return GAD_OK;
    GAD_REQUIRE(state, GAD_ERR_NULL, "point_state_pack: null pointer (state)");
    hipLaunchKernelGGL(point_state_pack_kernel, dim3(gad_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, (long long)src_stride,
                       sel, A, lead, n_lead, lead_flag, n, total, state);
    GAD_CHECK_LAUNCH("point_state_pack");
    return GAD_OK;
}
