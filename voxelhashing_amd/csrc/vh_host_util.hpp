// vh_host_util.hpp -- error plumbing shared by the launchers and host classes.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/vh_api.h"
#include "../../include/vh_owners.hpp"

// the host classes throw: an error code of the C ABI, or a HIP error, with the name of what failed
inline void check(int code, const char* what)
{
    if (code != 0) throw vh::Error(code, std::string(what) + ": " + vh_error_string(code));
}
inline void checkHip(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw vh::Error(-(int)e, std::string(what) + ": " + hipGetErrorString(e));
}

// C-ABI convention: 0 ok, <0 = -(hipError_t), >0 = VH_ERR_*
#define VH_HIP(expr)                                 \
    do {                                             \
        hipError_t vh_e_ = (expr);                   \
        if (vh_e_ != hipSuccess) return -(int)vh_e_; \
    } while (0)

#define VH_TRY(expr)                 \
    do {                             \
        int vh_r_ = (expr);          \
        if (vh_r_ != 0) return vh_r_; \
    } while (0)

static inline int vh_last_launch_error()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

// Is the row-major 4x4 T a rigid transform?  Finite entries, the last row (0, 0, 0, 1), a rotation orthonormal to 1e-4
// with a positive determinant: VH_OK, or VH_ERR_BAD_ARGUMENT.
static inline int vh_rigid_or_refuse(const double* T)
{
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(T[k])) return VH_ERR_BAD_ARGUMENT;
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return VH_ERR_BAD_ARGUMENT;
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r][c] = T[4 * r + c];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double dot = (R[0][a] * R[0][b] + R[1][a] * R[1][b]) + R[2][a] * R[2][b];
            if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-4)) return VH_ERR_BAD_ARGUMENT;
        }
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    return det > 0.0 ? VH_OK : VH_ERR_BAD_ARGUMENT;
}

// Timing one launch by the dispatch's own begin / end time stamps (what rocprofv3's kernel trace reports), instead of a
// pair of event records around it (each record costs the queue a few microseconds and a pair reads 5-7 us more than the
// kernel it brackets: 8.3 against 5.9 us for the fused integrate pass at cfg2).  vh_time_next_launch() arms the calling
// thread; the next launch that goes through VH_LAUNCH_TIMED uses hipExtLaunchKernel with the two events, and
// hipEventElapsedTime(start, stop) is then that kernel's duration.  Declared in include/vh_api.h.
bool vh_take_launch_events(hipEvent_t* start, hipEvent_t* stop);

#include <hip/hip_ext.h>
#define VH_LAUNCH_TIMED(kernel, grid, block, stream, ...)                                            \
    do {                                                                                             \
        hipEvent_t vh_e0_ = nullptr, vh_e1_ = nullptr;                                               \
        if (vh_take_launch_events(&vh_e0_, &vh_e1_))                                                 \
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, vh_e0_, vh_e1_, 0, __VA_ARGS__); \
        else                                                                                         \
            kernel<<<grid, block, 0, stream>>>(__VA_ARGS__);                                         \
    } while (0)
