// rgba_ab.hip -- the A/B baseline of tools/rgba_ab.py, and nothing else: the two per-picture colour kernels
// as the library had them before the batched ones (color.inc), verbatim, with entry points that launch
// them once per frame the way the single-stream C entry points did. Built by the tool into tools/build/.
#include <hip/hip_runtime.h>
#include <stdint.h>
#define DEV __device__ __forceinline__

__global__ __launch_bounds__(256) void rgba_to_i420_kernel(const uint8_t *__restrict__ rgba, int w, int h, uint8_t *__restrict__ out) {
    // one thread per 2x2 block
    int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    int cw = w / 2;
    if (bx >= cw || by >= h / 2) return;
    uint8_t *Y = out, *U = out + (size_t)w * h, *V = U + (size_t)cw * (h / 2);
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        const uint8_t *p = rgba + ((size_t)(2 * by + dy) * w + 2 * bx) * 4;
        uint2 px = *(const uint2 *)p;  // two RGBA pixels
        int r0 = px.x & 255, g0 = (px.x >> 8) & 255, b0 = (px.x >> 16) & 255;
        int r1 = px.y & 255, g1 = (px.y >> 8) & 255, b1 = (px.y >> 16) & 255;
        uint8_t y0 = (uint8_t)(((66 * r0 + 129 * g0 + 25 * b0 + 128) >> 8) + 16);
        uint8_t y1 = (uint8_t)(((66 * r1 + 129 * g1 + 25 * b1 + 128) >> 8) + 16);
        *(uint16_t *)&Y[(size_t)(2 * by + dy) * w + 2 * bx] = (uint16_t)(y0 | (y1 << 8));
        if (dy == 0) {
            U[(size_t)by * cw + bx] = (uint8_t)((uint8_t)((-38 * r0 - 74 * g0 + 112 * b0 + 128) >> 8) + 128);
            V[(size_t)by * cw + bx] = (uint8_t)((uint8_t)((112 * r0 - 94 * g0 - 18 * b0 + 128) >> 8) + 128);
        }
    }
}

// Saturate before the shift: clip1(x >> 8) == min(max(x, 0), 65535) >> 8. Written this way on
// purpose: hipcc (ROCm 7.2, gfx950) selects v_ashr_pk_u8_i32 for the "shift, saturate to u8, pack
// two bytes" form and then treats the instruction's untouched upper 16 bits as zero, corrupting the
// B/A bytes (toolchain notes). The clamp-first form never matches that pattern.
DEV uint32_t sat_shr8(int x) { return (uint32_t)min(max(x, 0), 65535) >> 8; }
DEV uint32_t yuv_px(int y, int cb, int cr) {
    const int c = 298 * (y - 16);
    return sat_shr8(c + 409 * cr + 128) | (sat_shr8(c - 100 * cb - 208 * cr + 128) << 8) | (sat_shr8(c + 516 * cb + 128) << 16) |
           0xff000000u;
}
__global__ __launch_bounds__(256) void i420_to_rgba_kernel(const uint8_t *__restrict__ Yp, const uint8_t *__restrict__ Up,
                                                           const uint8_t *__restrict__ Vp, int w, int h, int ys, int uvs,
                                                           uint8_t *__restrict__ rgba) {
    // one thread per 2 horizontally adjacent pixels (they share one chroma sample); 8-byte store
    int x2 = (blockIdx.x * blockDim.x + threadIdx.x) * 2, row = blockIdx.y;
    if (x2 >= w || row >= h) return;
    const int cb = Up[(size_t)(row / 2) * uvs + x2 / 2] - 128, cr = Vp[(size_t)(row / 2) * uvs + x2 / 2] - 128;
    const uint32_t p0 = yuv_px(Yp[(size_t)row * ys + x2], cb, cr);
    uint32_t *dst = (uint32_t *)(rgba + ((size_t)row * w + x2) * 4);
    if (x2 + 1 < w) *(uint2 *)dst = make_uint2(p0, yuv_px(Yp[(size_t)row * ys + x2 + 1], cb, cr));
    else dst[0] = p0;
}

// n tight frames back to back, one launch per frame on the stream
extern "C" int rgba_ab_parent_rgba_to_i420(void *d_i420, const void *d_rgba, int w, int h, int n, void *stream) {
    const size_t fr = (size_t)w * h * 4, fi = (size_t)w * h * 3 / 2;
    const dim3 g((w / 2 + 255) / 256, h / 2);
    (void)hipGetLastError();
    for (int f = 0; f < n; f++)
        hipLaunchKernelGGL(rgba_to_i420_kernel, g, dim3(256), 0, (hipStream_t)stream, (const uint8_t *)d_rgba + f * fr, w, h,
                           (uint8_t *)d_i420 + f * fi);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int rgba_ab_parent_i420_to_rgba(void *d_rgba, const void *d_i420, int w, int h, int n, void *stream) {
    const size_t fr = (size_t)w * h * 4, fi = (size_t)w * h * 3 / 2;
    const dim3 g(((w + 1) / 2 + 255) / 256, h);
    (void)hipGetLastError();
    for (int f = 0; f < n; f++) {
        const uint8_t *Y = (const uint8_t *)d_i420 + f * fi, *U = Y + (size_t)w * h, *V = U + (size_t)(w / 2) * (h / 2);
        hipLaunchKernelGGL(i420_to_rgba_kernel, g, dim3(256), 0, (hipStream_t)stream, Y, U, V, w, h, w, w / 2, (uint8_t *)d_rgba + f * fr);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
