// rt_engine.cpp -- the part of the C ABI (include/rt_engine.h) that belongs to no scene: status and errors, the
// memManager surface, and the constants of a frame. The scene is rt_scene.cpp, its cached tables rt_scene_tables.cpp,
// its resting-view tables rt_scene_rest.cpp, the launches rt_render.cpp, the post passes rt_post.cpp, the rayTrace shim
// rt_shim.cpp, the rt_debug_* entry points rt_debug.cpp.
//
// Reference interface replaced here:
//   memManager / check_cuda      /root/reference/memManager.h:11-18, memManager.cpp:3-22
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "rt_internal.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static char g_last_error[512] = "";
static int g_soft_errors = 0;

void rt_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}

int rt_hip_fail(hipError_t e, const char *expr, const char *file, int line)
{
    rt_set_error("HIP error = %u (%s) at %s:%d '%s'", (unsigned)e, hipGetErrorString(e), file, line, expr);
    (void)hipGetLastError();   // clear the sticky error so later calls can proceed
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? RT_ERR_NO_DEVICE : RT_ERR_HIP;
}

extern "C" const char *rt_last_error(void) { return g_last_error; }
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }
extern "C" int rt_set_soft_errors(int on)
{
    const int old = g_soft_errors;
    g_soft_errors = on ? 1 : 0;
    return old;
}
extern "C" int rt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// check_cuda, memManager.cpp:3-11
extern "C" void rt_check(int err, const char *expr, const char *file, int line)
{
    if (err) {
        fprintf(stderr, "HIP error = %u at %s:%d '%s' \n", (unsigned)err, file, line, expr);
        rt_set_error("HIP error = %u at %s:%d '%s'", (unsigned)err, file, line, expr);
        if (g_soft_errors) return;
        (void)hipDeviceReset();
        exit(99);
    }
}
#define checkHipErrors(val) rt_check((int)(val), #val, __FILE__, __LINE__)

// memManager::operator new / delete, memManager.cpp:12-22
extern "C" void *rt_managed_alloc(size_t len)
{
    void *ptr = nullptr;
    checkHipErrors(hipMallocManaged(&ptr, len ? len : 1));
    checkHipErrors(hipDeviceSynchronize());
    return ptr;
}
extern "C" void rt_managed_free(void *ptr)
{
    if (!ptr) return;
    rt_shim_forget(ptr);   // a sprite / mesh re-created at the same address must be uploaded again
    checkHipErrors(hipDeviceSynchronize());
    (void)hipFree(ptr);
}
// ---------------------------------------------------------------------------
// sample positions (build-defined extension; n = 1 is the reference's +0.5)
// ---------------------------------------------------------------------------
extern "C" int rt_sample_offset(int k, int n, double *ox, double *oy)
{
    if (n < 1 || k < 0 || k >= n || !ox || !oy) return RT_ERR_INVALID;
    int g = 1;
    while (g * g < n) ++g;   // stratified g x g grid, cell centres
    *ox = ((double)(k % g) + 0.5) / (double)g;
    *oy = ((double)(k / g) + 0.5) / (double)g;
    return RT_OK;
}

extern "C" float rt_default_aspect(void)
{
    return (float)std::tan((90 * 0.5 * 3.1415) / 180);   // kernel.cu:1701
}
