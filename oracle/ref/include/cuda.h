/* host stand-in: everything lives in cuda_runtime.h */
#pragma once
#include "cuda_runtime.h"
