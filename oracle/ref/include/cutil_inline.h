/* host stand-in for the SDK's cutil_inline.h: the runtime stand-in plus the error-check macros, which only evaluate */
#pragma once
#include "cuda_runtime.h"
#define cutilSafeCall(call) ((void)(call))
#define cutilCheckMsg(msg) ((void)0)
#define cutilSafeCallNoSync(call) ((void)(call))
