/*
 * cuda_runtime.h -- host stand-in, written for this project from the CUDA
 * programming guide's documented semantics.  It is just enough for the
 * reference's voxel-hashing sources to compile as plain host C++ (with
 * -D__CUDACC__) so that oracle/ref/vh_ref_wrap.cpp can run their device
 * functions and kernels serially on the CPU.
 *
 * Contract (the oracle's, see oracle/vh_oracle.c):
 *   - kernels run one workgroup after the other, blocks z, y, x, and within a
 *     workgroup one thread after the other, threads z, y, x (vhr_launch below).
 *     A workgroup whose threads reach __syncthreads runs them as cooperative
 *     fibers (oracle/ref/vhr_launch.cpp): each thread runs up to the barrier,
 *     and when all have arrived they resume, in the same order.  Atomics are
 *     plain read-modify-writes; __shared__ is `static` (one workgroup at a time);
 *   - rsqrtf is 1/sqrtf (correctly rounded), not the device's approximation;
 *   - textures use point filtering, unnormalised coordinates, clamp addressing.
 * Float -> int conversions are whatever the host compiler emits for a C++ cast
 * (x86 cvttss2si: out of range and NaN give INT_MIN); the device saturates.
 */
#ifndef VHR_CUDA_RUNTIME_H
#define VHR_CUDA_RUNTIME_H

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>

using std::abs;

/* ---- declaration qualifiers ---- */
#define __host__
#define __device__
#define __global__
#define __constant__
#define __shared__ static
#define __forceinline__ inline
#define __noinline__
#define __align__(n) __attribute__((aligned(n)))
#define CUDART_VERSION 5000

/* ---- vector types (CUDA's sizes and alignments) ---- */
#define VHR_VEC2(T, N, A) struct __align__(A) N##2 { T x, y; }; \
    inline N##2 make_##N##2(T x, T y) { N##2 r; r.x = x; r.y = y; return r; }
#define VHR_VEC3(T, N) struct N##3 { T x, y, z; }; \
    inline N##3 make_##N##3(T x, T y, T z) { N##3 r; r.x = x; r.y = y; r.z = z; return r; }
#define VHR_VEC4(T, N, A) struct __align__(A) N##4 { T x, y, z, w; }; \
    inline N##4 make_##N##4(T x, T y, T z, T w) { N##4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
#define VHR_VEC1(T, N) struct N##1 { T x; }; inline N##1 make_##N##1(T x) { N##1 r; r.x = x; return r; }

typedef unsigned char uchar_t_;
VHR_VEC1(signed char, char) VHR_VEC2(signed char, char, 2) VHR_VEC3(signed char, char) VHR_VEC4(signed char, char, 4)
VHR_VEC1(unsigned char, uchar) VHR_VEC2(unsigned char, uchar, 2) VHR_VEC3(unsigned char, uchar) VHR_VEC4(unsigned char, uchar, 4)
VHR_VEC1(short, short) VHR_VEC2(short, short, 4) VHR_VEC3(short, short) VHR_VEC4(short, short, 8)
VHR_VEC1(unsigned short, ushort) VHR_VEC2(unsigned short, ushort, 4) VHR_VEC3(unsigned short, ushort) VHR_VEC4(unsigned short, ushort, 8)
VHR_VEC1(int, int) VHR_VEC2(int, int, 8) VHR_VEC3(int, int) VHR_VEC4(int, int, 16)
VHR_VEC1(unsigned int, uint) VHR_VEC2(unsigned int, uint, 8) VHR_VEC3(unsigned int, uint) VHR_VEC4(unsigned int, uint, 16)
VHR_VEC1(float, float) VHR_VEC2(float, float, 8) VHR_VEC3(float, float) VHR_VEC4(float, float, 16)
VHR_VEC1(double, double) VHR_VEC2(double, double, 16) VHR_VEC3(double, double) VHR_VEC4(double, double, 16)

/* The host compiler the reference was built with (MSVC) binds a temporary to a non-const reference, and the unary
 * minus of the vector-math header takes one; these overloads serve the temporaries, with the same component negation. */
inline float2 operator-(const float2& a) { return make_float2(-a.x, -a.y); }
inline float3 operator-(const float3& a) { return make_float3(-a.x, -a.y, -a.z); }
inline float4 operator-(const float4& a) { return make_float4(-a.x, -a.y, -a.z, -a.w); }

struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
    dim3(uint3 v) : x(v.x), y(v.y), z(v.z) {}
};

/* ---- built-in variables: one emulated thread at a time ---- */
extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

/* One workgroup of the current launch (blockIdx set): every thread in order, threads z, y, x.  The first thread runs
 * on a fiber; if it returns without reaching a barrier, the others run one after the other on the caller's stack
 * (no fiber).  If it stops at __syncthreads, every thread gets a fiber and the workgroup runs barrier by barrier.
 * A barrier reached by only some of the threads aborts.  vhr_launch.cpp. */
typedef void (*vhr_thread_fn)(void*);
void vhr_run_workgroup(vhr_thread_fn fn, void* ctx, dim3 block);
void vhr_barrier();

template <class F> inline void vhr_call(void* f) { (*static_cast<F*>(f))(); }

/* Runs every workgroup of a launch in order: blocks z, y, x (vhr_run_workgroup).  The arguments of a launch are
 * converted to the kernel's parameter types as those of a function call are (CUDA programming guide, execution
 * configuration: "the arguments to the function are passed as in a normal call"), so a literal NULL becomes a null
 * pointer of the parameter's type: the parameter types are taken from the kernel, never deduced from the arguments. */
template <class T> struct vhr_identity { typedef T type; };
template <class... P>
inline void vhr_launch(dim3 grid, dim3 block, void (*kernel)(P...), const typename vhr_identity<P>::type&... args)
{
    gridDim = grid;
    blockDim = block;
    auto body = [&]() { kernel(args...); };
    for (unsigned int bz = 0; bz < grid.z; bz++)
    for (unsigned int by = 0; by < grid.y; by++)
    for (unsigned int bx = 0; bx < grid.x; bx++) {
        blockIdx.x = bx; blockIdx.y = by; blockIdx.z = bz;
        vhr_run_workgroup(&vhr_call<decltype(body)>, &body, block);
    }
}

inline void __syncthreads() { vhr_barrier(); }
inline void __threadfence() {}

/* ---- bit casts ---- */
inline float __int_as_float(int v) { float f; memcpy(&f, &v, 4); return f; }
inline int __float_as_int(float v) { int i; memcpy(&i, &v, 4); return i; }
inline float __uint_as_float(unsigned int v) { float f; memcpy(&f, &v, 4); return f; }
inline unsigned int __float_as_uint(float v) { unsigned int i; memcpy(&i, &v, 4); return i; }
inline float asfloat(unsigned int v) { return __uint_as_float(v); }
inline float asfloat(int v) { return __int_as_float(v); }

/* ---- math: the overloads CUDA's math API offers on the device ---- */
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
inline unsigned int min(int a, unsigned int b) { return min((unsigned int)a, b); }
inline unsigned int max(int a, unsigned int b) { return max((unsigned int)a, b); }
inline unsigned int min(unsigned int a, int b) { return min(a, (unsigned int)b); }
inline unsigned int max(unsigned int a, int b) { return max(a, (unsigned int)b); }
inline long long min(long long a, long long b) { return a < b ? a : b; }
inline long long max(long long a, long long b) { return a > b ? a : b; }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline double min(float a, double b) { return fmin((double)a, b); }
inline double max(float a, double b) { return fmax((double)a, b); }
inline double min(double a, float b) { return fmin(a, (double)b); }
inline double max(double a, float b) { return fmax(a, (double)b); }
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline float __fdividef(float a, float b) { return a / b; }
inline float __saturatef(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : (x == x ? x : 0.0f)); }

/* ---- atomics, sequential (one emulated thread runs at a time) ---- */
#define VHR_ATOMICS(T) \
    inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; } \
    inline T atomicSub(T* p, T v) { T o = *p; *p = o - v; return o; } \
    inline T atomicExch(T* p, T v) { T o = *p; *p = v; return o; } \
    inline T atomicMin(T* p, T v) { T o = *p; *p = o < v ? o : v; return o; } \
    inline T atomicMax(T* p, T v) { T o = *p; *p = o > v ? o : v; return o; }
VHR_ATOMICS(int)
VHR_ATOMICS(unsigned int)
VHR_ATOMICS(unsigned long long)
inline float atomicAdd(float* p, float v) { float o = *p; *p = o + v; return o; }
inline float atomicExch(float* p, float v) { float o = *p; *p = v; return o; }
inline int atomicCAS(int* p, int cmp, int v) { int o = *p; if (o == cmp) *p = v; return o; }
inline unsigned int atomicCAS(unsigned int* p, unsigned int cmp, unsigned int v) { unsigned int o = *p; if (o == cmp) *p = v; return o; }
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long cmp, unsigned long long v) { unsigned long long o = *p; if (o == cmp) *p = v; return o; }

/* ---- runtime API: host memory behind "device" pointers ---- */
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaMemcpyDefault };
typedef void* cudaStream_t;
typedef void* cudaEvent_t;
template <class T> inline cudaError_t cudaMalloc(T** p, size_t n) { *p = (T*)calloc(1, n ? n : 1); return *p ? cudaSuccess : 2; }
inline cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }
inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) { memcpy(d, s, n); return cudaSuccess; }
inline cudaError_t cudaMemset(void* d, int v, size_t n) { memset(d, v, n); return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "cuda stand-in error"; }

/* ---- textures: a cudaArray is a host image; tex2D reads it with point filtering ---- */
enum cudaChannelFormatKind { cudaChannelFormatKindSigned, cudaChannelFormatKindUnsigned, cudaChannelFormatKindFloat, cudaChannelFormatKindNone };
struct cudaChannelFormatDesc { int x, y, z, w; cudaChannelFormatKind f; };
inline cudaChannelFormatDesc cudaCreateChannelDesc(int x, int y, int z, int w, cudaChannelFormatKind f)
{
    cudaChannelFormatDesc d; d.x = x; d.y = y; d.z = z; d.w = w; d.f = f; return d;
}
struct cudaArray { const void* data; size_t width, height, elemBytes; };
inline cudaError_t cudaMallocArray(cudaArray** a, const cudaChannelFormatDesc* d, size_t w, size_t h, unsigned int = 0)
{
    *a = new cudaArray();
    (*a)->elemBytes = (size_t)(d->x + d->y + d->z + d->w) / 8;
    (*a)->data = calloc(w * h, (*a)->elemBytes);
    (*a)->width = w; (*a)->height = h;
    return cudaSuccess;
}
inline cudaError_t cudaFreeArray(cudaArray* a) { if (a) { free((void*)a->data); delete a; } return cudaSuccess; }

enum cudaTextureType { cudaTextureType1D = 1, cudaTextureType2D = 2, cudaTextureType3D = 3 };
enum cudaTextureReadMode { cudaReadModeElementType, cudaReadModeNormalizedFloat };
enum cudaTextureFilterMode { cudaFilterModePoint, cudaFilterModeLinear };
enum cudaTextureAddressMode { cudaAddressModeWrap, cudaAddressModeClamp, cudaAddressModeMirror, cudaAddressModeBorder };

template <class T, int dim = 1, enum cudaTextureReadMode mode = cudaReadModeElementType>
struct texture {
    const cudaArray* array = nullptr;
    int normalized = 0;
    cudaTextureFilterMode filterMode = cudaFilterModePoint;
    cudaTextureAddressMode addressMode[3] = { cudaAddressModeClamp, cudaAddressModeClamp, cudaAddressModeClamp };
};

template <class T, int dim, enum cudaTextureReadMode mode>
inline cudaError_t cudaBindTextureToArray(texture<T, dim, mode>& t, const cudaArray* a, const cudaChannelFormatDesc&)
{
    t.array = a;
    return cudaSuccess;
}
template <class T, int dim, enum cudaTextureReadMode mode>
inline cudaError_t cudaUnbindTexture(texture<T, dim, mode>& t) { t.array = nullptr; return cudaSuccess; }

/* point filtering on unnormalised coordinates: texel floor(x), floor(y), clamped to the image */
template <class T, int dim, enum cudaTextureReadMode mode>
inline T tex2D(const texture<T, dim, mode>& t, float x, float y)
{
    const cudaArray* a = t.array;
    if (!a || t.filterMode != cudaFilterModePoint || t.normalized) abort();
    long ix = (long)floorf(x), iy = (long)floorf(y);
    if (ix < 0) ix = 0;
    if (iy < 0) iy = 0;
    if (ix > (long)a->width - 1) ix = (long)a->width - 1;
    if (iy > (long)a->height - 1) iy = (long)a->height - 1;
    return ((const T*)a->data)[(size_t)iy * a->width + (size_t)ix];
}

#endif
