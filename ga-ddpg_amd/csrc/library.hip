// What every unit of libgaddpg links against (host only, no kernel): the thread's error string, the timing slot and stream
// priorities, the grid-rows hint, the ABI version, the name of the last GEMM route, and the geometry units' option block.
#include "common.hpp"
#include <stdarg.h>
#include <string.h>

static thread_local char g_err[512] = "";
static thread_local unsigned long long* g_timing_slot = nullptr;

unsigned long long* gad_take_timing_slot() {
    unsigned long long* p = g_timing_slot;
    g_timing_slot = nullptr;
    return p;
}

// wavefront issue priority per stream (gaddpg.h: gad_stream_priority): a small table, written before the steps start
static void* g_prio_stream[8];
static int g_prio_val[8];
static int g_prio_n = 0;
extern "C" int gad_stream_priority(void* stream, int prio) {
    GAD_REQUIRE(prio >= 0 && prio <= 3, GAD_ERR_SHAPE, "stream_priority: priority %d outside 0..3", prio);
    for (int i = 0; i < g_prio_n; ++i)
        if (g_prio_stream[i] == stream) { g_prio_val[i] = prio; return GAD_OK; }
    if (prio == 0) return GAD_OK;
    GAD_REQUIRE(g_prio_n < 8, GAD_ERR_SHAPE, "stream_priority: more than 8 prioritised streams");
    g_prio_stream[g_prio_n] = stream;
    g_prio_val[g_prio_n++] = prio;
    return GAD_OK;
}
unsigned long long* gad_take_timing_slot(void* stream) {
    size_t v = reinterpret_cast<size_t>(gad_take_timing_slot());
    for (int i = 0; i < g_prio_n; ++i)
        if (g_prio_stream[i] == stream) v |= (size_t)g_prio_val[i];
    return reinterpret_cast<unsigned long long*>(v);
}

extern "C" int gad_timing_slot(void* slot) {
    GAD_REQUIRE((reinterpret_cast<size_t>(slot) & 7) == 0, GAD_ERR_SHAPE, "timing_slot: the slot must be 8-byte aligned");
    g_timing_slot = static_cast<unsigned long long*>(slot);
    return GAD_OK;
}

// Grid-size hint for the next tiled gad_gemm_fwd / gad_gemm_dx launch of this thread (see gaddpg.h)
static thread_local int g_grid_rows = 0;
int gad_take_grid_rows() {
    const int r = g_grid_rows;
    g_grid_rows = 0;
    return gad_deterministic() ? 0 : r;          // the mode sizes every grid by the row capacity: hints cannot regroup partial sums
}
extern "C" int gad_grid_rows_hint(const int32_t* rows_host, void* /*stream: unused, plan calls pass one*/) {
    g_grid_rows = rows_host ? *rows_host : 0;
    return GAD_OK;
}

extern "C" int gad_wall_clock_khz(void) {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
}
void gad_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* gad_last_error(void) { return g_err; }
extern "C" int gad_abi_version(void) { return 12; }

const char* g_gad_last_kernel = "";
extern "C" const char* gad_last_kernel(void) { return g_gad_last_kernel; }

// the geometry units' options (common.hpp: GeometryOptions); gad_set_option of gemm.hip tries them after the GEMM options, any int is taken
GeometryOptions g_geo_opt;
static const struct { const char* name; int GeometryOptions::*member; } k_geo_options[] = {
    {"bq_cells", &GeometryOptions::bq_cells}, {"bq_grid", &GeometryOptions::bq_grid},
    {"tnn_grid", &GeometryOptions::tnn_grid}, {"fps_cfg", &GeometryOptions::fps_cfg},
};
void gad_geometry_set_option(const char* name, int value, int* found) {
    for (const auto& o : k_geo_options)
        if (!strcmp(name, o.name)) { g_geo_opt.*o.member = value; *found = 1; }
}
