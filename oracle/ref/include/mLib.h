/* host stand-in: only the two macros the ray-cast header's host code uses */
#pragma once
#include "cuda_runtime.h"
#define MLIB_CUDA_SAFE_CALL(call) ((void)(call))
#define MLIB_CUDA_SAFE_FREE(p) do { if (p) { cudaFree(p); (p) = NULL; } } while (0)
