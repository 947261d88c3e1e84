// vh_view.hip -- the shaded view of the model: DX11RGBDRenderer::RenderDepthMap (a depth map drawn as a mesh) and
// DX11PhongLighting::render as compute passes for gfx950, their launcher-level C ABI (include/vh_api.h) and the host
// classes RGBDRenderer / PhongLighting (include/vh.hpp).
//
// Reference behaviour: DepthSensingCUDA/Shaders/RGBDRenderer.hlsl (RGBDRendererGS, ComputeQuadVertex,
// RGBDRendererRawDepthPS), Shaders/PhongLighting.hlsl (PhongPS) and the D3D11 default rasterizer state.  The reference
// is D3D11 code; there is no CUDA to follow, so the rules are the ones DESIGN.md section 4 ("Rendering") pins down and
// tests/view_render.py restates.
//
//   k_view_raster        one lane per depth-map quad: both triangles, coverage by int64 edge functions on D3D's
//                        1/256-pixel grid, a 64-bit atomicMin of (float_bits(z) << 32 | primitive id) per covered pixel.
//                        A triangle whose clipped box holds more than kLargeBox pixels is appended to a list instead.
//   k_view_raster_large  one workgroup per listed triangle, its 256 lanes over the box.
//   k_view_resolve       one lane per screen pixel: the winning primitive's vertices again (the same device function),
//                        the four maps, and the key / list reset, so the next view needs no clear launch.
//   k_view_resolve_depth the same lane and reset, render target 0 only (the source depth): CUDARGBDSensor's remap of
//                        the depth map into the colour camera (s_bUseCameraCalibration).
//   k_phong              one lane per pixel: PhongPS, float4 and/or RGBA8.
//
// MUST be compiled with -ffp-contract=off: the restatement is bit-exact only with every multiply and add rounded.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/vh.hpp"
#include "vh_device.hpp"
#include "vh_host_util.hpp"

namespace {

constexpr float kDepthWorldMin = 0.1f; // DEPTH_WORLD_MIN / MAX of RGBDRenderer.hlsl:3-4
constexpr float kDepthWorldMax = 8.0f;
constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint64_t kLargeBox = 64;     // pixels of a clipped box above which a triangle goes to the second phase
constexpr float kGuard = 268435456.0f; // 2^20 px on the 1/256 grid: a snapped coordinate beyond it drops the triangle
constexpr uint32_t kLargeBlocks = 1024;

using vhd::cdiv;

struct ViewVertex {
    float X, Y, z; // screen position (pixels, y down) and D3D depth
    float depth;   // fDepth: the source depth
    float4 pos, normal, color;
};

struct ViewTri {
    int64_t x[3], y[3]; // snapped to 1/256 px
    int64_t area;       // twice the signed area on that grid; > 0 is front (clockwise on screen)
};

__device__ inline float load_depth(const float* depth, const VhViewParams& p, uint32_t x, uint32_t y)
{
    // Texture2D::Load outside the image returns 0; x - 1 at 0 wraps, as the shader's uint does
    return (x < p.depthWidth && y < p.depthHeight) ? depth[(size_t)y * p.depthWidth + x] : 0.0f;
}

// mul(v, M) of the shader with M read column-major = M v with M as the host holds it; the sum runs j = 0..3
__device__ inline float4 mat_vec(const float* M, float4 v)
{
    return make_float4(M[0] * v.x + M[1] * v.y + M[2] * v.z + M[3] * v.w, M[4] * v.x + M[5] * v.y + M[6] * v.z + M[7] * v.w,
                       M[8] * v.x + M[9] * v.y + M[10] * v.z + M[11] * v.w, M[12] * v.x + M[13] * v.y + M[14] * v.z + M[15] * v.w);
}

// getWorldSpacePosition, hlsl:67-77
__device__ inline float4 world_position(const float* depth, const VhViewParams& p, uint32_t x, uint32_t y)
{
    const float d = load_depth(depth, p, x, y);
    float4 c = mat_vec(p.intrinsicInverse, make_float4((float)x * d, (float)y * d, d, d));
    c = make_float4(c.x, c.y, c.w, 1.0f);
    const float4 w = mat_vec(p.modelview, c);
    return make_float4(w.x / w.w, w.y / w.w, w.z / w.w, w.w / w.w);
}

// ComputeQuadVertex, hlsl:79-111, then the viewport transform
__device__ inline ViewVertex view_vertex(const float* depth, const float4* color, const VhViewParams& p, uint32_t x, uint32_t y)
{
    ViewVertex v;
    v.depth = load_depth(depth, p, x, y);
    const float4 cc = world_position(depth, p, x, y);
    const float4 mc = world_position(depth, p, x - 1, y);
    const float4 cm = world_position(depth, p, x, y - 1);
    const float4 cp = world_position(depth, p, x, y + 1);
    const float4 pc = world_position(depth, p, x + 1, y);
    const float ax = cp.x - cm.x, ay = cp.y - cm.y, az = cp.z - cm.z;
    const float bx = pc.x - mc.x, by = pc.y - mc.y, bz = pc.z - mc.z;
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    v.normal = make_float4(nx / len, ny / len, nz / len, 1.0f);
    const float4 clip = mat_vec(p.intrinsicNew, make_float4(cc.x, cc.y, cc.z, 1.0f));
    const float px = clip.x / clip.z, py = clip.y / clip.z;
    const float fx = (px / (float)(p.screenWidth - 1)) * 2.0f - 1.0f;
    const float fy = 1.0f - (py / (float)(p.screenHeight - 1)) * 2.0f;
    v.z = (clip.z - kDepthWorldMin) / (kDepthWorldMax - kDepthWorldMin);
    v.X = (fx + 1.0f) * 0.5f * (float)p.screenWidth;
    v.Y = (1.0f - fy) * 0.5f * (float)p.screenHeight;
    v.pos = cc;
    v.color = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (color && x < p.depthWidth && y < p.depthHeight) v.color = color[(size_t)y * p.depthWidth + x];
    return v;
}

// The three vertices of primitive `prim` in the order the strip gives them: quad q = prim / 2 emits (x, y+1), (x, y),
// (x+1, y+1), (x+1, y); triangle 0 is (v0, v1, v2), triangle 1 is (v2, v1, v3).  Raster and resolve both call this.
__device__ inline void view_triangle_vertices(const float* depth, const float4* color, const VhViewParams& p, uint32_t prim, ViewVertex v[3])
{
    const uint32_t q = prim >> 1, x = q % p.depthWidth, y = q / p.depthWidth;
    if (prim & 1u) {
        v[0] = view_vertex(depth, color, p, x + 1, y + 1);
        v[1] = view_vertex(depth, color, p, x, y);
        v[2] = view_vertex(depth, color, p, x + 1, y);
    } else {
        v[0] = view_vertex(depth, color, p, x, y + 1);
        v[1] = view_vertex(depth, color, p, x, y);
        v[2] = view_vertex(depth, color, p, x + 1, y + 1);
    }
}

// RGBDRendererGS's drop rules, hlsl:122-137
__device__ inline bool view_quad_kept(const float* depth, const VhViewParams& p, uint32_t x, uint32_t y)
{
    const float d0 = load_depth(depth, p, x, y), d1 = load_depth(depth, p, x, y + 1);
    const float d2 = load_depth(depth, p, x + 1, y), d3 = load_depth(depth, p, x + 1, y + 1);
    if (d0 <= kDepthWorldMin || d1 <= kDepthWorldMin || d2 <= kDepthWorldMin || d3 <= kDepthWorldMin) return false;
    const float minf = -INFINITY;
    if (d0 == minf || d1 == minf || d2 == minf || d3 == minf) return false;
    const float dmax = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3));
    const float dmin = fminf(fminf(d0, d1), fminf(d2, d3));
    const float d = 0.5f * (dmax + dmin);
    return !(dmax - dmin > p.depthThreshOffset + p.depthThreshLin * d);
}

// snap to the 1/256 grid, guard band, back-face cull (D3D11 default: CULL_BACK, clockwise front)
__device__ inline bool view_setup(const ViewVertex v[3], ViewTri& t)
{
    for (int k = 0; k < 3; k++) {
        const float sx = rintf(v[k].X * 256.0f), sy = rintf(v[k].Y * 256.0f);
        if (!(fabsf(sx) <= kGuard) || !(fabsf(sy) <= kGuard)) return false;
        t.x[k] = (int64_t)sx;
        t.y[k] = (int64_t)sy;
    }
    t.area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
    return t.area > 0;
}

// pixels whose centre can lie in the triangle, clipped to the screen; false if none
__device__ inline bool view_box(const ViewTri& t, uint32_t sw, uint32_t sh, int32_t& x0, int32_t& x1, int32_t& y0, int32_t& y1)
{
    const int64_t mnx = min(t.x[0], min(t.x[1], t.x[2])), mxx = max(t.x[0], max(t.x[1], t.x[2]));
    const int64_t mny = min(t.y[0], min(t.y[1], t.y[2])), mxy = max(t.y[0], max(t.y[1], t.y[2]));
    // centre of pixel i is i * 256 + 128: first i with centre >= min, last with centre <= max
    const int64_t lx = max((int64_t)0, -((128 - mnx) >> 8)), hx = min((int64_t)sw - 1, (mxx - 128) >> 8);
    const int64_t ly = max((int64_t)0, -((128 - mny) >> 8)), hy = min((int64_t)sh - 1, (mxy - 128) >> 8);
    if (lx > hx || ly > hy) return false;
    x0 = (int32_t)lx; x1 = (int32_t)hx; y0 = (int32_t)ly; y1 = (int32_t)hy;
    return true;
}

// edge functions at (px, py) with the top-left rule; e[k] is the weight of vertex k (the edge opposite it)
__device__ inline bool view_cover(const ViewTri& t, int64_t px, int64_t py, int64_t e[3])
{
    for (int k = 0; k < 3; k++) {
        const int a = k == 2 ? 0 : k + 1, b = k == 0 ? 2 : k - 1;
        const int64_t dx = t.x[b] - t.x[a], dy = t.y[b] - t.y[a];
        e[k] = dx * (py - t.y[a]) - dy * (px - t.x[a]);
        const bool topLeft = dy < 0 || (dy == 0 && dx > 0);
        if (!(e[k] > 0 || (e[k] == 0 && topLeft))) return false;
    }
    return true;
}

__device__ inline void view_bary(const ViewTri& t, const int64_t e[3], float b[3])
{
    const float area = (float)t.area;
    for (int k = 0; k < 3; k++) b[k] = (float)e[k] / area;
}

__device__ inline float interp(float a0, float a1, float a2, const float b[3]) { return a0 * b[0] + a1 * b[1] + a2 * b[2]; }
__device__ inline float4 interp4(float4 a0, float4 a1, float4 a2, const float b[3])
{
    return make_float4(interp(a0.x, a1.x, a2.x, b), interp(a0.y, a1.y, a2.y, b), interp(a0.z, a1.z, a2.z, b), interp(a0.w, a1.w, a2.w, b));
}

__device__ inline void raster_pixel(const ViewTri& t, const float z3[3], int32_t i, int32_t j, uint32_t prim, uint64_t* keys, uint32_t sw)
{
    int64_t e[3];
    if (!view_cover(t, (int64_t)i * 256 + 128, (int64_t)j * 256 + 128, e)) return;
    float b[3];
    view_bary(t, e, b);
    const float z = interp(z3[0], z3[1], z3[2], b) + 0.0f; // -0 -> +0, so that the key orders as z does
    if (!(z >= 0.0f && z < 1.0f)) return;                  // clip to [0, w], then LESS against the 1.0 clear
    atomicMin(reinterpret_cast<unsigned long long*>(keys) + (size_t)j * sw + i, ((unsigned long long)__float_as_uint(z) << 32) | prim);
}

__global__ __launch_bounds__(256) void k_view_raster(const float* depth, VhViewParams p, uint64_t* keys, uint32_t* large)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.depthWidth * p.depthHeight) return;
    if (!view_quad_kept(depth, p, q % p.depthWidth, q / p.depthWidth)) return;
    for (uint32_t t = 0; t < 2; t++) {
        const uint32_t prim = 2 * q + t;
        ViewVertex v[3];
        view_triangle_vertices(depth, nullptr, p, prim, v);
        ViewTri tri;
        int32_t x0, x1, y0, y1;
        if (!view_setup(v, tri) || !view_box(tri, p.screenWidth, p.screenHeight, x0, x1, y0, y1)) continue;
        if ((uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1) > kLargeBox) {
            large[1 + atomicAdd(large, 1u)] = prim; // at most 2 w h entries: the list has room for every primitive
            continue;
        }
        const float z3[3] = { v[0].z, v[1].z, v[2].z };
        for (int32_t j = y0; j <= y1; j++)
            for (int32_t i = x0; i <= x1; i++) raster_pixel(tri, z3, i, j, prim, keys, p.screenWidth);
    }
}

__global__ __launch_bounds__(256) void k_view_raster_large(const float* depth, VhViewParams p, uint64_t* keys, const uint32_t* large)
{
    const uint32_t n = large[0];
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t prim = large[1 + k];
        ViewVertex v[3];
        view_triangle_vertices(depth, nullptr, p, prim, v);
        ViewTri tri;
        int32_t x0, x1, y0, y1;
        if (!view_setup(v, tri) || !view_box(tri, p.screenWidth, p.screenHeight, x0, x1, y0, y1)) continue;
        const float z3[3] = { v[0].z, v[1].z, v[2].z };
        const uint32_t bw = (uint32_t)(x1 - x0 + 1), npix = bw * (uint32_t)(y1 - y0 + 1);
        for (uint32_t m = threadIdx.x; m < npix; m += blockDim.x)
            raster_pixel(tri, z3, x0 + (int32_t)(m % bw), y0 + (int32_t)(m / bw), prim, keys, p.screenWidth);
    }
}

__global__ __launch_bounds__(256) void k_view_resolve(const float* depth, const float4* color, VhViewParams p, uint64_t* keys, uint32_t* large,
                                                      float* outDepth, float4* outPos, float4* outNormal, float4* outColor)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) large[0] = 0; // k_view_raster_large, the list's last reader, has finished
    if (idx >= p.screenWidth * p.screenHeight) return;
    const uint64_t key = keys[idx];
    const float minf = -INFINITY;
    float d = minf;
    float4 pos = make_float4(minf, minf, minf, 1.0f), nrm = pos, col = pos;
    if (key != kEmptyKey) {
        keys[idx] = kEmptyKey;
        ViewVertex v[3];
        view_triangle_vertices(depth, color, p, (uint32_t)key, v);
        ViewTri tri;
        view_setup(v, tri);
        int64_t e[3];
        view_cover(tri, (int64_t)(idx % p.screenWidth) * 256 + 128, (int64_t)(idx / p.screenWidth) * 256 + 128, e);
        float b[3];
        view_bary(tri, e, b);
        d = interp(v[0].depth, v[1].depth, v[2].depth, b);
        pos = interp4(v[0].pos, v[1].pos, v[2].pos, b);
        nrm = interp4(v[0].normal, v[1].normal, v[2].normal, b);
        col = interp4(v[0].color, v[1].color, v[2].color, b);
    }
    outDepth[idx] = d;
    outPos[idx] = pos;
    outNormal[idx] = nrm;
    outColor[idx] = col;
}

// Render target 0 alone (RGBDRendererRawDepthPS's res.depth = In.fDepth, clear -inf), written straight into the
// caller's map.  The vertices come from the same device function as above; with no colour and only X, Y and the source
// depth read, the compiler drops the neighbour loads and the normal, so a covered pixel costs three depth-map taps.
__global__ __launch_bounds__(256) void k_view_resolve_depth(const float* depth, VhViewParams p, uint64_t* keys, uint32_t* large, float* outDepth)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) large[0] = 0; // k_view_raster_large, the list's last reader, has finished
    if (idx >= p.screenWidth * p.screenHeight) return;
    const uint64_t key = keys[idx];
    float d = -INFINITY;
    if (key != kEmptyKey) {
        keys[idx] = kEmptyKey;
        ViewVertex v[3];
        view_triangle_vertices(depth, nullptr, p, (uint32_t)key, v);
        ViewTri tri;
        view_setup(v, tri);
        int64_t e[3];
        view_cover(tri, (int64_t)(idx % p.screenWidth) * 256 + 128, (int64_t)(idx / p.screenWidth) * 256 + 128, e);
        float b[3];
        view_bary(tri, e, b);
        d = interp(v[0].depth, v[1].depth, v[2].depth, b);
    }
    outDepth[idx] = d;
}

// ---------------------------------------------------------------------------
// PhongPS, Shaders/PhongLighting.hlsl:49-86
// ---------------------------------------------------------------------------

__device__ inline float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline float3 normalize3(float3 v)
{
    const float l = sqrtf(dot3(v, v));
    return make_float3(v.x / l, v.y / l, v.z / l);
}

__device__ inline uint32_t unorm8(float c)
{
    if (!(c == c)) return 0u;
    return (uint32_t)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f);
}

__global__ __launch_bounds__(256) void k_phong(const float4* positions, const float4* normals, const float4* colors, uint32_t n, uint32_t useMaterial,
                                               VhPhongLight L, float4* out4, uint32_t* outRGBA8, uint32_t alphaRule)
{
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float4 p4 = positions[idx], n4 = normals[idx], c4 = colors[idx];
    const float minf = -INFINITY;
    float4 res = make_float4(minf, minf, minf, minf);
    if (p4.x != minf && c4.x != minf && n4.x != minf) {
        const float3 position = make_float3(p4.x, p4.y, p4.z), normal = make_float3(n4.x, n4.y, n4.z);
        const float3 ld = normalize3(make_float3(L.lightDirection[0], L.lightDirection[1], L.lightDirection[2]));
        const float3 eyeDir = normalize3(position);
        const float3 i = make_float3(-ld.x, -ld.y, -ld.z);
        const float t = 2.0f * dot3(normal, i); // reflect(i, n) = i - 2 dot(n, i) n
        const float3 R = normalize3(make_float3(i.x - t * normal.x, i.y - t * normal.y, i.z - t * normal.z));
        const float diff = fmaxf(dot3(normal, i), 0.0f);
        const float spec = powf(fmaxf(dot3(R, eyeDir), 0.0f), L.materialShininess);
        float r[4];
        if (useMaterial) {
            const float material[4] = { c4.x, c4.y, c4.z, 1.0f };
            for (int k = 0; k < 4; k++) r[k] = (L.lightDiffuse[k] * material[k] * diff + L.lightSpecular[k] * L.materialSpecular[k] * spec) * 2.0f;
        } else {
            for (int k = 0; k < 4; k++)
                r[k] = L.lightAmbient[k] * L.materialAmbient[k] + L.lightDiffuse[k] * L.materialDiffuse[k] * diff + L.lightSpecular[k] * L.materialSpecular[k] * spec;
        }
        res = make_float4(r[0], r[1], r[2], r[3]);
    }
    if (out4) out4[idx] = res;
    if (outRGBA8) {
        const uint32_t r = unorm8(res.x), g = unorm8(res.y), b = unorm8(res.z);
        const uint32_t a = (alphaRule && (r | g | b)) ? 255u : unorm8(res.w);
        outRGBA8[idx] = r | (g << 8) | (b << 16) | (a << 24);
    }
}

bool viewParamsValid(const VhViewParams* p)
{
    return p && p->depthWidth > 0 && p->depthHeight > 0 && p->screenWidth >= 2 && p->screenHeight >= 2 &&
           (uint64_t)p->depthWidth * p->depthHeight < (1ull << 30) && (uint64_t)p->screenWidth * p->screenHeight < (1ull << 31);
}


} // namespace

extern "C" {

uint32_t vh_view_large_list_words(uint32_t width, uint32_t height) { return 2u * width * height + 1u; }

int vh_view_raster(const float* d_depth, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList, vhStream_t stream)
{
    if (!d_depth || !d_keys || !d_largeList || !viewParamsValid(params)) return VH_ERR_BAD_ARGUMENT;
    const hipStream_t s = (hipStream_t)stream;
    k_view_raster<<<cdiv(params->depthWidth * params->depthHeight, 256u), 256, 0, s>>>(d_depth, *params, d_keys, d_largeList);
    VH_TRY(vh_last_launch_error());
    k_view_raster_large<<<kLargeBlocks, 256, 0, s>>>(d_depth, *params, d_keys, d_largeList);
    return vh_last_launch_error();
}

int vh_view_resolve(const float* d_depth, const float* d_color4, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList,
                    float* d_outDepth, float* d_outPosition4, float* d_outNormal4, float* d_outColor4, vhStream_t stream)
{
    if (!d_depth || !d_color4 || !d_keys || !d_largeList || !d_outDepth || !d_outPosition4 || !d_outNormal4 || !d_outColor4 || !viewParamsValid(params))
        return VH_ERR_BAD_ARGUMENT;
    k_view_resolve<<<cdiv(params->screenWidth * params->screenHeight, 256u), 256, 0, (hipStream_t)stream>>>(
        d_depth, reinterpret_cast<const float4*>(d_color4), *params, d_keys, d_largeList, d_outDepth, reinterpret_cast<float4*>(d_outPosition4),
        reinterpret_cast<float4*>(d_outNormal4), reinterpret_cast<float4*>(d_outColor4));
    return vh_last_launch_error();
}

int vh_view_resolve_depth(const float* d_depth, const VhViewParams* params, uint64_t* d_keys, uint32_t* d_largeList, float* d_outDepth, vhStream_t stream)
{
    if (!d_depth || !d_keys || !d_largeList || !d_outDepth || d_outDepth == d_depth || !viewParamsValid(params)) return VH_ERR_BAD_ARGUMENT;
    k_view_resolve_depth<<<cdiv(params->screenWidth * params->screenHeight, 256u), 256, 0, (hipStream_t)stream>>>(d_depth, *params, d_keys, d_largeList,
                                                                                                                   d_outDepth);
    return vh_last_launch_error();
}

int vh_phong(const float* d_positions4, const float* d_normals4, const float* d_colors4, uint32_t numPixels, int useMaterial, const VhPhongLight* light,
             float* d_out4, uint8_t* d_outRGBA8, int alphaRule, vhStream_t stream)
{
    if (!d_positions4 || !d_normals4 || !d_colors4 || !light || (!d_out4 && !d_outRGBA8)) return VH_ERR_BAD_ARGUMENT;
    if (numPixels == 0) return VH_OK;
    k_phong<<<cdiv(numPixels, 256u), 256, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(d_positions4), reinterpret_cast<const float4*>(d_normals4), reinterpret_cast<const float4*>(d_colors4), numPixels,
        useMaterial == 1 ? 1u : 0u, *light, reinterpret_cast<float4*>(d_out4), reinterpret_cast<uint32_t*>(d_outRGBA8), alphaRule ? 1u : 0u);
    return vh_last_launch_error();
}

} // extern "C"

// ---------------------------------------------------------------------------
// host classes
// ---------------------------------------------------------------------------

RGBDRenderer::RGBDRenderer(vhStream_t stream) : m_stream(stream) {}

RGBDRenderer::~RGBDRenderer() = default;

void RGBDRenderer::resize(unsigned int width, unsigned int height, unsigned int screenWidth, unsigned int screenHeight)
{
    const hipStream_t s = (hipStream_t)m_stream;
    if (width != m_width || height != m_height) { // OnResize: the list is sized by the depth map
        d_largeList = vh::deviceAlloc<uint32_t>(vh_view_large_list_words(width, height), "RGBDRenderer: list");
        checkHip(hipMemsetAsync(d_largeList.get(), 0, sizeof(uint32_t), s), "RGBDRenderer: list");
        m_width = width;
        m_height = height;
    }
    if (screenWidth != m_screenWidth || screenHeight != m_screenHeight) {
        const size_t n = (size_t)screenWidth * screenHeight;
        d_keys = vh::deviceAlloc<uint64_t>(n, "RGBDRenderer: keys");
        checkHip(hipMemsetAsync(d_keys.get(), 0xff, sizeof(uint64_t) * n, s), "RGBDRenderer: keys");
        d_depth = vh::deviceAlloc<float>(n, "RGBDRenderer: depth");
        d_positions = vh::deviceAlloc<float>(4 * n, "RGBDRenderer: positions");
        d_normals = vh::deviceAlloc<float>(4 * n, "RGBDRenderer: normals");
        d_colors = vh::deviceAlloc<float>(4 * n, "RGBDRenderer: colors");
        m_screenWidth = screenWidth;
        m_screenHeight = screenHeight;
    }
}

void RGBDRenderer::RenderDepthMap(const float* d_depthMap, const float* d_colorMap, unsigned int width, unsigned int height,
                                  const vh::mat4f& intrinsicDepthToWorld, const vh::mat4f& modelview, const vh::mat4f& intrinsicWorldToDepth,
                                  unsigned int screenWidth, unsigned int screenHeight, float depthThreshOffset, float depthThreshLin)
{
    VhViewParams p;
    std::memset(&p, 0, sizeof(p));
    std::memcpy(p.intrinsicInverse, intrinsicDepthToWorld.m, sizeof(p.intrinsicInverse));
    std::memcpy(p.modelview, modelview.m, sizeof(p.modelview));
    std::memcpy(p.intrinsicNew, intrinsicWorldToDepth.m, sizeof(p.intrinsicNew));
    p.depthWidth = width;
    p.depthHeight = height;
    p.screenWidth = screenWidth;
    p.screenHeight = screenHeight;
    p.depthThreshOffset = depthThreshOffset;
    p.depthThreshLin = depthThreshLin;
    if (!d_depthMap || !d_colorMap || !viewParamsValid(&p)) throw vh::Error(VH_ERR_BAD_ARGUMENT, "RenderDepthMap: bad arguments");
    resize(width, height, screenWidth, screenHeight);
    check(vh_view_raster(d_depthMap, &p, d_keys.get(), d_largeList.get(), m_stream), "RenderDepthMap: raster");
    check(vh_view_resolve(d_depthMap, d_colorMap, &p, d_keys.get(), d_largeList.get(), d_depth.get(), d_positions.get(), d_normals.get(), d_colors.get(), m_stream), "RenderDepthMap: resolve");
}

PhongLighting::PhongLighting(const VhPhongLight& light, vhStream_t stream) : m_light(light), m_stream(stream) {}

PhongLighting::~PhongLighting() = default;

void PhongLighting::render(const float* d_positions, const float* d_normals, const float* d_colorsIn, bool useMaterial, unsigned int width,
                           unsigned int height, bool rgba8)
{
    const unsigned int n = width * height;
    if (n != m_numPixels) {
        d_colors = vh::deviceAlloc<float>(4 * (size_t)n, "PhongLighting: colors");
        d_rgba8 = vh::deviceAlloc<uint8_t>(4 * (size_t)n, "PhongLighting: rgba8");
        m_numPixels = n;
    }
    check(vh_phong(d_positions, d_normals, d_colorsIn, n, useMaterial ? 1 : 0, &m_light, d_colors.get(), rgba8 ? d_rgba8.get() : nullptr, 1, m_stream),
          "PhongLighting::render");
}
