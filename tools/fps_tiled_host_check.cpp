// Stand-alone check of the host side of gad_fps_tiled, gad_ball_query_grid, gad_three_nn_grid and the observation entry points
// (gad_backproject_depth, gad_cloud_gather_affine, gad_point_state_pack) (include/gaddpg.h section A) for a
// sanitizer build: the workspace sizes, every refusing argument path and the calls with nothing to do, none of which launches
// anything -- so it runs on a machine without a GPU.  (The expectations on the two grid entry points are those of
// tests/test_ball_query_grid_host.py and tests/test_three_nn_grid_host.py, those on the observation entry points of
// tests/test_point_state_host.py.)  It also runs gad_set_option's table over every GEMM option and the first refusals of the GEMM
// entry points (the expectations of tests/test_abi.py).  Build it together
// with the library's sources, host code instrumented, and run it as it is:
//
//   cd ga-ddpg_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -munsafe-fp-atomics \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/fps_tiled_host_check.cpp library.hip fps.hip ball_query.hip group.hip interpolate.hip point_grid.hip \
//       observe.hip gemm.hip gemm_fwd.hip gemm_dx.hip gemm_dw.hip gemm_bwd.hip coord_grad.hip layers.hip losses.hip optim.hip plan.hip \
//       -o fps_tiled_host_check
//
// Exit status 0 and "ok" on success; a failed expectation prints its line and exits 1.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gaddpg.h"

static int g_failed = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            printf("line %d: %s   (last error: %s)\n", __LINE__, #cond, gad_last_error()); \
            g_failed = 1;                                                              \
        }                                                                              \
    } while (0)

int main() {
    float* p = reinterpret_cast<float*>(0x1000);             // never dereferenced: every call below is refused or has nothing to do
    int32_t* q = reinterpret_cast<int32_t*>(0x2000);
    void* ws = reinterpret_cast<void*>(0x3000);
    const int cap = 1 << 22;

    EXPECT(gad_fps_tiled_workspace_bytes(1, 1, 1, 0) >= 1 * 4 + 1 * 8);
    EXPECT(gad_fps_tiled_workspace_bytes(2, 12000, 5000, 0) >= 2ll * 12000 * 4 + 2ll * 5000 * 8);
    EXPECT(gad_fps_tiled_workspace_bytes(2, 12000, 5001, 3) > gad_fps_tiled_workspace_bytes(2, 12000, 5000, 3));
    EXPECT(gad_fps_tiled_workspace_bytes(2, 12100, 5000, 3) > gad_fps_tiled_workspace_bytes(2, 12000, 5000, 3));
    EXPECT(gad_fps_tiled_workspace_bytes(512, cap, 1 << 30, cap / 4096) >= 512ll * cap * 4 + 512ll * (1 << 30) * 8);      // 64-bit arithmetic
    EXPECT(gad_fps_tiled_workspace_bytes(0, 64, 8, 0) == 0);
    EXPECT(gad_fps_tiled_workspace_bytes(1, cap + 1, 8, 0) == GAD_ERR_SHAPE && strstr(gad_last_error(), "N=4194305"));
    EXPECT(gad_fps_tiled_workspace_bytes(1, 64, 8, 65) == GAD_ERR_SHAPE && strstr(gad_last_error(), "groups=65"));
    EXPECT(gad_fps_tiled_workspace_bytes(1, 2147483647, 2147483647, 0) == GAD_ERR_SHAPE);
    EXPECT(gad_fps_tiled_workspace_bytes(-1, 64, 8, 0) == GAD_ERR_SHAPE);

    EXPECT(gad_fps_tiled(nullptr, 1, 64, 8, 0, q, nullptr, ws, nullptr) == GAD_ERR_NULL && strstr(gad_last_error(), "null pointer"));
    EXPECT(gad_fps_tiled(p, 1, 64, 8, 0, nullptr, nullptr, ws, nullptr) == GAD_ERR_NULL);
    EXPECT(gad_fps_tiled(p, 1, 64, 8, 0, q, nullptr, nullptr, nullptr) == GAD_ERR_NULL && strstr(gad_last_error(), "workspace"));
    EXPECT(gad_fps_tiled(p, 1, 64, 8, 0, q, nullptr, reinterpret_cast<void*>(0x3004), nullptr) == GAD_ERR_SHAPE &&
           strstr(gad_last_error(), "aligned"));
    EXPECT(gad_fps_tiled(p, -1, 64, 8, 0, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE);
    EXPECT(gad_fps_tiled(p, 1, 0, 8, 0, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE);
    EXPECT(gad_fps_tiled(p, 1, 64, -1, 0, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE);
    EXPECT(gad_fps_tiled(p, 1, cap + 1, 8, 0, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE && strstr(gad_last_error(), "N=4194305"));
    EXPECT(gad_fps_tiled(p, 1, 64, 8, 65, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE && strstr(gad_last_error(), "groups=65"));
    EXPECT(gad_fps_tiled(p, 1, 64, 8, -3, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE && strstr(gad_last_error(), "groups=-3"));
    EXPECT(gad_fps_tiled(p, 2147483647, cap, 8, cap, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE && strstr(gad_last_error(), "overflows"));
    EXPECT(gad_fps_tiled(p, 4096, cap, 8, 2048, q, nullptr, ws, nullptr) == GAD_ERR_SHAPE && strstr(gad_last_error(), "overflows"));
    EXPECT(gad_fps_tiled(p, 0, 64, 8, 0, q, nullptr, nullptr, nullptr) == GAD_OK);          // nothing to sample: no launch
    EXPECT(gad_fps_tiled(p, 7, 64, 0, 3, q, nullptr, nullptr, nullptr) == GAD_OK);
    // the one-workgroup entry point's refusals, for comparison (unchanged)
    EXPECT(gad_furthest_point_sampling(p, 1, 64, 65, q, nullptr, nullptr) == GAD_ERR_SHAPE);
    EXPECT(gad_furthest_point_sampling(p, 1, 16384, 16384, q, nullptr, nullptr) == GAD_ERR_SHAPE);

    // gad_ball_query_grid(new_xyz, xyz, B, N, M, radius, nsample, idx, cnt, workspace, stream)
    auto bq = [&](const float* c, const float* x, int B, int N, int M, int ns, int32_t* idx, void* w) {
        return gad_ball_query_grid(c, x, B, N, M, 0.1f, ns, idx, nullptr, w, nullptr);
    };
    auto says = [](const char* what) { return strstr(gad_last_error(), what) != nullptr; };
    void* odd = reinterpret_cast<void*>(0x3004);
    EXPECT(bq(nullptr, p, 1, 5000, 8, 4, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bq(p, nullptr, 1, 5000, 8, 4, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bq(p, p, 1, 5000, 8, 4, nullptr, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bq(p, p, 1, 5000, 8, 4, q, nullptr) == GAD_ERR_NULL && says("workspace"));
    EXPECT(bq(p, p, 1, 5000, 8, 4, q, odd) == GAD_ERR_SHAPE && says("aligned"));
    EXPECT(bq(p, p, -1, 5000, 8, 4, q, ws) == GAD_ERR_SHAPE && says("B=-1"));
    EXPECT(bq(p, p, 1, 0, 8, 4, q, ws) == GAD_ERR_SHAPE && says("N=0"));
    EXPECT(bq(p, p, 1, -3, 8, 4, q, ws) == GAD_ERR_SHAPE && says("N=-3"));
    EXPECT(bq(p, p, 1, 5000, -2, 4, q, ws) == GAD_ERR_SHAPE && says("M=-2"));
    EXPECT(bq(p, p, 1, 5000, 8, 0, q, ws) == GAD_ERR_SHAPE && says("nsample=0"));
    EXPECT(bq(p, p, 1, 5000, 8, -1, q, ws) == GAD_ERR_SHAPE && says("nsample=-1"));
    EXPECT(bq(p, p, 1, 800000000, 8, 4, q, ws) == GAD_ERR_SHAPE && says("overflows"));      // 3 * N, B * N, the grid of B * M centroids
    EXPECT(bq(p, p, 1024, 1 << 21, 8, 4, q, ws) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(bq(p, p, 1 << 10, 5000, 1 << 16, 4, q, ws) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(bq(p, p, 0, 5000, 8, 4, q, nullptr) == GAD_OK);                                    // nothing to search: no launch
    EXPECT(bq(p, p, 2, 5000, 0, 4, q, nullptr) == GAD_OK);
    EXPECT(gad_ball_query_grid_workspace_bytes(1, 5000, 8, 16) >= 5000 * 24);
    EXPECT(gad_ball_query_grid_workspace_bytes(3, 70000, 64, 200) >= gad_ball_query_grid_workspace_bytes(1, 70000, 64, 200));
    EXPECT(gad_ball_query_grid_workspace_bytes(256, 1 << 22, 64, 16) > 1ll << 32);          // more than 32 bits before the shape is
    EXPECT(gad_ball_query_grid_workspace_bytes(1, 0, 8, 4) == GAD_ERR_SHAPE && says("N=0"));
    EXPECT(gad_ball_query_grid_workspace_bytes(-1, 64, 8, 4) == GAD_ERR_SHAPE && says("B=-1"));
    EXPECT(gad_ball_query_grid_workspace_bytes(1, 64, 8, 0) == GAD_ERR_SHAPE && says("nsample=0"));
    EXPECT(gad_ball_query_grid_workspace_bytes(1, 800000000, 8, 4) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(gad_ball_query_grid_workspace_bytes(1 << 10, 5000, 1 << 16, 4) == GAD_ERR_SHAPE && says("overflows"));

    // gad_three_nn_grid(unknown, known, B, n, m, dist2, idx, stats, workspace, stream)
    auto nn = [&](const float* u, const float* k, int B, int n, int m, float* d, int32_t* idx, void* w) {
        return gad_three_nn_grid(u, k, B, n, m, d, idx, nullptr, w, nullptr);
    };
    EXPECT(nn(nullptr, p, 1, 8, 5000, p, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(nn(p, nullptr, 1, 8, 5000, p, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(nn(p, p, 1, 8, 5000, nullptr, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(nn(p, p, 1, 8, 5000, p, nullptr, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(nn(p, p, 1, 8, 5000, p, q, nullptr) == GAD_ERR_NULL && says("workspace"));
    EXPECT(nn(p, p, 1, 8, 5000, p, q, odd) == GAD_ERR_SHAPE && says("aligned"));
    EXPECT(nn(p, p, -1, 8, 5000, p, q, ws) == GAD_ERR_SHAPE && says("B=-1"));
    EXPECT(nn(p, p, 1, -8, 5000, p, q, ws) == GAD_ERR_SHAPE && says("n=-8"));
    EXPECT(nn(p, p, 1, 8, -3, p, q, ws) == GAD_ERR_SHAPE && says("m=-3"));
    EXPECT(nn(p, p, 1, 8, 0, p, q, ws) == GAD_ERR_SHAPE && says("no known point"));
    EXPECT(nn(p, p, 1, 8, 800000000, p, q, ws) == GAD_ERR_SHAPE && says("overflows"));       // 3 * m, B * m, B * n, B itself
    EXPECT(nn(p, p, 1024, 8, 1 << 21, p, q, ws) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(nn(p, p, 1024, 1 << 21, 64, p, q, ws) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(nn(p, p, 65536, 8, 64, p, q, ws) == GAD_ERR_SHAPE && says("65535"));
    EXPECT(nn(p, p, 0, 8, 5000, p, q, nullptr) == GAD_OK);                                    // no query: no launch, and m may be 0
    EXPECT(nn(p, p, 2, 0, 5000, p, q, nullptr) == GAD_OK);
    EXPECT(gad_three_nn_grid(p, p, 2, 0, 0, p, q, q, nullptr, nullptr) == GAD_OK);
    EXPECT(gad_three_nn_grid_workspace_bytes(1, 0, 5000) == gad_three_nn_grid_workspace_bytes(1, 1 << 20, 5000));
    EXPECT(gad_three_nn_grid_workspace_bytes(1, 8, 5000) == gad_ball_query_grid_workspace_bytes(1, 5000, 8, 16));   // one grid, one layout
    EXPECT(gad_three_nn_grid_workspace_bytes(3, 64, 70000) >= gad_three_nn_grid_workspace_bytes(1, 64, 70000));
    EXPECT(gad_three_nn_grid_workspace_bytes(256, 64, 1 << 22) > 1ll << 32);
    EXPECT(gad_three_nn_grid_workspace_bytes(1, 8, 0) == GAD_ERR_SHAPE && says("no known point"));
    EXPECT(gad_three_nn_grid_workspace_bytes(-1, 8, 64) == GAD_ERR_SHAPE && says("B=-1"));
    EXPECT(gad_three_nn_grid_workspace_bytes(1, -8, 64) == GAD_ERR_SHAPE && says("n=-8"));
    EXPECT(gad_three_nn_grid_workspace_bytes(1, 8, -64) == GAD_ERR_SHAPE && says("m=-64"));
    EXPECT(gad_three_nn_grid_workspace_bytes(1, 8, 800000000) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(gad_three_nn_grid_workspace_bytes(1024, 8, 1 << 21) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(gad_three_nn_grid_workspace_bytes(1024, 1 << 21, 64) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(gad_three_nn_grid_workspace_bytes(65536, 8, 64) == GAD_ERR_SHAPE && says("65535"));
    EXPECT(gad_three_nn_grid_workspace_bytes(2, 0, 0) > 0);                                   // nothing to search is no error

    // gad_backproject_depth(depth, depth_u16, depth_div, mask, A, B, H, W, xyz, count, pix, workspace, stream)
    const uint8_t* nomask = nullptr;
    auto bp = [&](const void* d, int u16, float div, const float* A, int B, int H, int W, float* xyz, int32_t* cnt, void* w) {
        return gad_backproject_depth(d, u16, div, nomask, A, B, H, W, xyz, cnt, nullptr, w, nullptr);
    };
    EXPECT(bp(nullptr, 0, 1.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bp(p, 0, 1.f, nullptr, 1, 8, 8, p, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bp(p, 0, 1.f, p, 1, 8, 8, nullptr, q, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bp(p, 0, 1.f, p, 1, 8, 8, p, nullptr, ws) == GAD_ERR_NULL && says("null pointer"));
    EXPECT(bp(p, 0, 1.f, p, 1, 8, 8, p, q, nullptr) == GAD_ERR_NULL && says("workspace"));
    EXPECT(bp(p, 0, 1.f, p, 1, 8, 8, p, q, odd) == GAD_ERR_SHAPE && says("aligned"));
    EXPECT(bp(reinterpret_cast<void*>(0x1002), 0, 1.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("element size"));
    EXPECT(bp(reinterpret_cast<void*>(0x1001), 1, 5000.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("element size"));
    EXPECT(bp(p, 1, 0.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("divisor"));
    EXPECT(bp(p, 1, -5000.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("divisor"));
    EXPECT(bp(p, 3, 1.f, p, 1, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("depth_u16=3"));
    EXPECT(bp(p, 0, 1.f, p, 1, 0, 8, p, q, ws) == GAD_ERR_SHAPE && says("outside 1..4096"));
    EXPECT(bp(p, 0, 1.f, p, 1, 8, 4097, p, q, ws) == GAD_ERR_SHAPE && says("outside 1..4096"));
    EXPECT(bp(p, 0, 1.f, p, -2, 8, 8, p, q, ws) == GAD_ERR_SHAPE && says("B=-2"));
    EXPECT(bp(p, 0, 1.f, p, 128, 4096, 4096, p, q, ws) == GAD_ERR_SHAPE && says("beyond 2^31"));
    EXPECT(bp(p, 0, 1.f, p, 2147483647, 1, 1, p, q, ws) == GAD_ERR_SHAPE && says("overflows"));
    EXPECT(bp(nullptr, 0, 1.f, nullptr, 0, 8, 8, nullptr, nullptr, nullptr) == GAD_OK);       // no image: no launch
    EXPECT(gad_backproject_depth_workspace_bytes(1, 112, 112) >= 13 * 4);
    EXPECT(gad_backproject_depth_workspace_bytes(127, 4096, 4096) >= 127ll * 16384 * 4);
    EXPECT(gad_backproject_depth_workspace_bytes(0, 8, 8) == 0);
    EXPECT(gad_backproject_depth_workspace_bytes(128, 4096, 4096) == GAD_ERR_SHAPE && says("beyond 2^31"));
    EXPECT(gad_backproject_depth_workspace_bytes(1, 4097, 8) == GAD_ERR_SHAPE && says("outside 1..4096"));
    EXPECT(gad_backproject_depth_workspace_bytes(1, 8, -1) == GAD_ERR_SHAPE && says("outside 1..4096"));

    // gad_cloud_gather_affine(src, src_stride, sel, A, B, n, dst, dst_stride, stream)
    EXPECT(gad_cloud_gather_affine(nullptr, 0, nullptr, nullptr, 1, 4, p, 0, nullptr) == GAD_ERR_NULL && says("(src)"));
    EXPECT(gad_cloud_gather_affine(p, 0, nullptr, nullptr, 1, 4, nullptr, 0, nullptr) == GAD_ERR_NULL && says("(dst)"));
    EXPECT(gad_cloud_gather_affine(p, -1, nullptr, nullptr, 1, 4, p, 0, nullptr) == GAD_ERR_SHAPE && says("src_stride=-1"));
    EXPECT(gad_cloud_gather_affine(p, 0, nullptr, nullptr, 1, 4, p, -1, nullptr) == GAD_ERR_SHAPE && says("dst_stride=-1"));
    EXPECT(gad_cloud_gather_affine(p, 0, nullptr, nullptr, -1, 4, p, 0, nullptr) == GAD_ERR_SHAPE && says("B=-1"));
    EXPECT(gad_cloud_gather_affine(p, 0, nullptr, nullptr, 1 << 16, 1 << 15, p, 0, nullptr) == GAD_ERR_SHAPE && says("beyond 2^31"));
    EXPECT(gad_cloud_gather_affine(nullptr, 0, nullptr, nullptr, 3, 0, nullptr, 0, nullptr) == GAD_OK);       // no point: no launch

    // gad_point_state_pack(src, src_stride, sel, A, lead, n_lead, lead_flag, B, n, state, stream)
    EXPECT(gad_point_state_pack(nullptr, 0, nullptr, nullptr, p, 6, 1.f, 1, 4, p, nullptr) == GAD_ERR_NULL && says("(src)"));
    EXPECT(gad_point_state_pack(p, 0, nullptr, nullptr, nullptr, 6, 1.f, 1, 4, p, nullptr) == GAD_ERR_NULL && says("(lead)"));
    EXPECT(gad_point_state_pack(p, 0, nullptr, nullptr, p, 6, 1.f, 1, 4, nullptr, nullptr) == GAD_ERR_NULL && says("(state)"));
    EXPECT(gad_point_state_pack(p, 0, nullptr, nullptr, p, -6, 1.f, 1, 4, p, nullptr) == GAD_ERR_SHAPE && says("n_lead=-6"));
    EXPECT(gad_point_state_pack(p, 0, nullptr, nullptr, p, 2147483647, 1.f, 1, 2147483647, p, nullptr) == GAD_ERR_SHAPE && says("beyond 2^31"));
    EXPECT(gad_point_state_pack(nullptr, 0, nullptr, nullptr, nullptr, 0, 1.f, 4, 0, nullptr, nullptr) == GAD_OK);   // no column: no launch

    // gad_set_option's table (gemm.hip): every GEMM option takes its default; out-of-range values fall back instead of being refused
    // (the expectations of tests/test_abi.py); defaults again at the end
    static const struct { const char* name; int def; } opts[20] = {
        {"mfma_split", 0}, {"deterministic", 0}, {"fwd_wide", 1}, {"dx_wide", 1}, {"dw_wide", 1}, {"bwd_fused", 1}, {"fwd_bn_prologue", 1},
        {"bwd_wide", 0}, {"bwd_wide_slab", 4}, {"dw_wide_wgs", 256}, {"skinny_nw", 8}, {"fwd_skinny", 1}, {"dx_skinny", 1}, {"dx_stream", 1},
        {"dw_skinny", 1}, {"dw_stream", 1}, {"fwd_stream", 1}, {"bwd_stream_wgs", 256}, {"fwd_stream_wgs", 256}, {"fwd_stream_l1_wgs", 256}};
    for (const auto& o : opts) EXPECT(gad_set_option(o.name, o.def) == GAD_OK);
    for (const char* name : {"bwd_stream_wgs", "fwd_stream_wgs", "fwd_stream_l1_wgs", "dw_wide_wgs", "bwd_wide_slab"})
        for (int v : {0, -5, 2147483647, 257}) EXPECT(gad_set_option(name, v) == GAD_OK);
    for (int v : {0, 3, 5, 16, -4, 4}) EXPECT(gad_set_option("skinny_nw", v) == GAD_OK);
    for (int v : {1, 7, -1, 0, 0}) EXPECT(gad_set_option("deterministic", v) == GAD_OK);      // 1 -> 0 releases the (empty) scratch
    for (int v : {-2147483647 - 1, 2147483647}) EXPECT(gad_set_option("mfma_split", v) == GAD_OK);
    EXPECT(gad_set_option("fwd_widee", 1) == GAD_ERR_SHAPE && says("unknown option 'fwd_widee'"));
    EXPECT(gad_set_option("", 1) == GAD_ERR_SHAPE && says("unknown option"));
    EXPECT(gad_set_option(nullptr, 1) == GAD_ERR_NULL && says("null name"));
    for (const auto& o : opts) EXPECT(gad_set_option(o.name, o.def) == GAD_OK);

    // the first checks of the GEMM entry points: refused before anything is launched
    gad_gemm_fwd_args fa;
    memset(&fa, 0, sizeof fa);
    EXPECT(gad_gemm_fwd(nullptr, nullptr) == GAD_ERR_NULL && says("null pointer"));
    fa.W = p; fa.zout = p; fa.n_groups = 7; fa.Kp = 8;
    EXPECT(gad_gemm_fwd(&fa, nullptr) == GAD_ERR_SHAPE && says("n_groups"));
    fa.n_groups = 1; fa.Kp = 12;
    EXPECT(gad_gemm_fwd(&fa, nullptr) == GAD_ERR_SHAPE && says("Kp=12"));
    gad_gemm_dx_args xa;
    memset(&xa, 0, sizeof xa);
    EXPECT(gad_gemm_dx(&xa, nullptr) == GAD_ERR_NULL && says("gemm_dx: null pointer"));
    EXPECT(gad_gemm_dx(nullptr, nullptr) == GAD_ERR_NULL);
    gad_gemm_dw_args wa;
    memset(&wa, 0, sizeof wa);
    EXPECT(gad_gemm_dw(nullptr, nullptr) == GAD_ERR_NULL && says("gemm_dw: null pointer"));
    EXPECT(gad_gemm_dw(&wa, nullptr) == GAD_ERR_NULL && says("gemm_dw: null pointer"));           // no gacc
    EXPECT(gad_gemm_bwd(nullptr, &wa, nullptr) == GAD_ERR_NULL && says("gemm_bwd: null pointer"));
    EXPECT(gad_gemm_bwd(&xa, nullptr, nullptr) == GAD_ERR_NULL && says("gemm_bwd: null pointer"));
    EXPECT(gad_gemm_dw_reduce(nullptr, &wa, nullptr) == GAD_ERR_NULL && says("gemm_dw_reduce: null pointer"));
    EXPECT(gad_gemm_dw_reduce(&xa, nullptr, nullptr) == GAD_ERR_NULL && says("gemm_dw_reduce: null pointer"));
    EXPECT(gad_gemm_dw_reduce(&xa, &wa, nullptr) == GAD_OK);                                        // no rows: nothing to reduce
    if (g_failed) return 1;
    printf("ok\n");
    return 0;
}
