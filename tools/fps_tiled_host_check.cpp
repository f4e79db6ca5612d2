// Stand-alone check of the host side of gad_fps_tiled (include/gaddpg.h section A) for a sanitizer build: the workspace size and
// every refusing argument path, none of which launches anything -- so it runs on a machine without a GPU.  Build it together
// with the library's sources, host code instrumented, and run it as it is:
//
//   cd ga-ddpg_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -munsafe-fp-atomics \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/fps_tiled_host_check.cpp geometry.hip gemm.hip layers.hip losses.hip optim.hip plan.hip -o fps_tiled_host_check
//
// Exit status 0 and "ok" on success; a failed expectation prints its line and exits 1.
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
    if (g_failed) return 1;
    printf("ok\n");
    return 0;
}
