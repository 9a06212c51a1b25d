// color.inc -- the wrapper's colour conversions at the edges of the codec (gfx950), batched: n frames of
// one geometry per launch.
//   rgba_to_i420_kernel : rgba_to_yuv (openh264_wrapper.cpp:22-40) -- BT.601 limited range,
//                         chroma from the top-left pixel of each 2x2 (no averaging), u8 wrap
//   i420_to_rgba_kernel : yuv_to_rgba_optimized (:150-195) -- integer BT.601, clamp, A = 255
//   dec_output_rgba_kernel : the same conversion as the batch decoder's per-frame read-out
// Pure per-pixel byte work, HBM bound (5.5 w h bytes a frame either way). One lane converts 8 adjacent
// pixels on 2 rows: two 16-byte RGBA accesses a row, one 8-byte Y access a row, one 4-byte U and V access.
// Lanes are consecutive 8-pixel units of the frame in raster order, so a wave covers contiguous 2 KB RGBA
// row segments. That vector form needs w % 8 == 0, a 16-byte aligned RGBA frame, 8-byte aligned Y rows and
// 4-byte aligned chroma rows; the kernel tests this per frame (tight I420 frames are w h 3/2 bytes apart,
// a multiple of 8 but not always of 16) and otherwise converts the lane's 8-pixel span as up to four 2x2
// blocks with byte accesses on the planes and 4-byte accesses on the RGBA pixels -- the same bytes.
// No access leaves its frame on either path.
namespace h264mi {

#define H264MI_COLOR_MAX_BLOCKS 2048  // 8 blocks of 256 on each of 256 CUs; the rest is a stride loop
#define H264MI_COLOR_MAX_FRAMES_Y 256

// One RGBA pixel (R | G << 8 | B << 16 | A << 24; alpha ignored) to Y, U, V
DEV uint32_t rgb_y(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16);
}
DEV uint32_t rgb_u(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)((uint8_t)((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128);
}
DEV uint32_t rgb_v(uint32_t p) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    return (uint8_t)((uint8_t)((112 * r - 94 * g - 18 * b + 128) >> 8) + 128);
}
DEV uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }

// n tight RGBA frames -> n tight I420 frames. Grid (blocks over a frame's units, frames), both capped.
__global__ __launch_bounds__(256) void rgba_to_i420_kernel(const uint8_t *__restrict__ rgba, uint8_t *__restrict__ out, int w, int h,
                                                           int n) {
    const int cw = w >> 1, upr = (w + 7) >> 3, units = upr * (h >> 1);  // 8x2-pixel units per row pair / per frame
    const size_t fin = (size_t)w * h * 4, fout = (size_t)w * h + 2 * (size_t)cw * (h >> 1);
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t *src = rgba + (size_t)f * fin;
        uint8_t *Y = out + (size_t)f * fout, *U = Y + (size_t)w * h, *V = U + (size_t)cw * (h >> 1);
        const bool vec = ((w & 7) | ((uintptr_t)src & 15) | ((uintptr_t)Y & 7) | ((uintptr_t)U & 3) | ((uintptr_t)V & 3)) == 0;
        for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
            const int by = u / upr, x = (u - by * upr) * 8;
            const uint8_t *p = src + ((size_t)(2 * by) * w + x) * 4;
            uint8_t *y = Y + (size_t)(2 * by) * w + x;
            const size_t c = (size_t)by * cw + (x >> 1);
            if (vec) {
                const uint4 a0 = *(const uint4 *)p, a1 = *(const uint4 *)(p + 16);
                const uint4 b0 = *(const uint4 *)(p + (size_t)w * 4), b1 = *(const uint4 *)(p + (size_t)w * 4 + 16);
                *(uint2 *)y = make_uint2(pack4(rgb_y(a0.x), rgb_y(a0.y), rgb_y(a0.z), rgb_y(a0.w)),
                                         pack4(rgb_y(a1.x), rgb_y(a1.y), rgb_y(a1.z), rgb_y(a1.w)));
                *(uint2 *)(y + w) = make_uint2(pack4(rgb_y(b0.x), rgb_y(b0.y), rgb_y(b0.z), rgb_y(b0.w)),
                                               pack4(rgb_y(b1.x), rgb_y(b1.y), rgb_y(b1.z), rgb_y(b1.w)));
                *(uint32_t *)(U + c) = pack4(rgb_u(a0.x), rgb_u(a0.z), rgb_u(a1.x), rgb_u(a1.z));
                *(uint32_t *)(V + c) = pack4(rgb_v(a0.x), rgb_v(a0.z), rgb_v(a1.x), rgb_v(a1.z));
            } else {
                for (int k = 0; k < 4 && x + 2 * k < w; k++) {  // one 2x2 block a step
                    const uint32_t *q0 = (const uint32_t *)p + 2 * k, *q1 = q0 + w;
                    const uint32_t p00 = q0[0];
                    y[2 * k] = (uint8_t)rgb_y(p00); y[2 * k + 1] = (uint8_t)rgb_y(q0[1]);
                    y[w + 2 * k] = (uint8_t)rgb_y(q1[0]); y[w + 2 * k + 1] = (uint8_t)rgb_y(q1[1]);
                    U[c + k] = (uint8_t)rgb_u(p00);
                    V[c + k] = (uint8_t)rgb_v(p00);
                }
            }
        }
    }
}

// Saturate before the shift: clip1(x >> 8) == min(max(x, 0), 65535) >> 8. Written this way on
// purpose: hipcc (ROCm 7.2, gfx950) selects v_ashr_pk_u8_i32 for the "shift, saturate to u8, pack
// two bytes" form and then treats the instruction's untouched upper 16 bits as zero, corrupting the
// B/A bytes (DESIGN.md §7, toolchain notes). The clamp-first form never matches that pattern.
DEV uint32_t sat_shr8(int x) { return (uint32_t)min(max(x, 0), 65535) >> 8; }
DEV uint32_t yuv_px(int y, int cb, int cr) {
    const int c = 298 * (y - 16);
    return sat_shr8(c + 409 * cr + 128) | (sat_shr8(c - 100 * cb - 208 * cr + 128) << 8) | (sat_shr8(c + 516 * cb + 128) << 16) |
           0xff000000u;
}
DEV int byte_of(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255); }
// 4 pixels of one row: luma bytes yy, chroma bytes k0 and k0 + 1 of ub / vb
DEV uint4 yuv_px4(uint32_t yy, uint32_t ub, uint32_t vb, int k0) {
    const int cb0 = byte_of(ub, k0) - 128, cr0 = byte_of(vb, k0) - 128, cb1 = byte_of(ub, k0 + 1) - 128, cr1 = byte_of(vb, k0 + 1) - 128;
    return make_uint4(yuv_px(byte_of(yy, 0), cb0, cr0), yuv_px(byte_of(yy, 1), cb0, cr0), yuv_px(byte_of(yy, 2), cb1, cr1),
                      yuv_px(byte_of(yy, 3), cb1, cr1));
}

// One w x h picture (even w and h; planes with strides ys / uvs) to a tight RGBA frame: the units
// u0, u0 + ustep, ... of the picture. Shared by the batched kernel and the decoder's read-out.
DEV void i420_to_rgba_picture(const uint8_t *__restrict__ Y, const uint8_t *__restrict__ U, const uint8_t *__restrict__ V, int ys, int uvs,
                              int w, int h, uint8_t *__restrict__ rgba, int u0, int ustep) {
    const int upr = (w + 7) >> 3, units = upr * (h >> 1);
    const bool vec = ((w & 7) | (ys & 7) | (uvs & 3) | ((uintptr_t)rgba & 15) | ((uintptr_t)Y & 7) | ((uintptr_t)U & 3) | ((uintptr_t)V & 3)) == 0;
    for (int u = u0; u < units; u += ustep) {
        const int by = u / upr, x = (u - by * upr) * 8;
        const uint8_t *y = Y + (size_t)(2 * by) * ys + x;
        const size_t c = (size_t)by * uvs + (x >> 1);
        uint8_t *d = rgba + ((size_t)(2 * by) * w + x) * 4;
        if (vec) {
            const uint2 y0 = *(const uint2 *)y, y1 = *(const uint2 *)(y + ys);
            const uint32_t ub = *(const uint32_t *)(U + c), vb = *(const uint32_t *)(V + c);
            *(uint4 *)d = yuv_px4(y0.x, ub, vb, 0);
            *(uint4 *)(d + 16) = yuv_px4(y0.y, ub, vb, 2);
            *(uint4 *)(d + (size_t)w * 4) = yuv_px4(y1.x, ub, vb, 0);
            *(uint4 *)(d + (size_t)w * 4 + 16) = yuv_px4(y1.y, ub, vb, 2);
        } else {
            for (int k = 0; k < 4 && x + 2 * k < w; k++) {  // one 2x2 block a step
                const int cb = U[c + k] - 128, cr = V[c + k] - 128;
                uint32_t *q0 = (uint32_t *)d + 2 * k, *q1 = q0 + w;
                q0[0] = yuv_px(y[2 * k], cb, cr); q0[1] = yuv_px(y[2 * k + 1], cb, cr);
                q1[0] = yuv_px(y[ys + 2 * k], cb, cr); q1[1] = yuv_px(y[ys + 2 * k + 1], cb, cr);
            }
        }
    }
}

// n pictures: frame f's planes are y / u / v + f * fstride, with row strides ys / uvs
struct I420Pics { const uint8_t *y, *u, *v; size_t fstride; int ys, uvs; };
__global__ __launch_bounds__(256) void i420_to_rgba_kernel(I420Pics p, int w, int h, int n, uint8_t *__restrict__ rgba) {
    for (int f = blockIdx.y; f < n; f += gridDim.y)
        i420_to_rgba_picture(p.y + f * p.fstride, p.u + f * p.fstride, p.v + f * p.fstride, p.ys, p.uvs, w, h, rgba + (size_t)f * w * h * 4,
                             blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// RGBA read-out of a batched decode call (H264MI_FMT_RGBA; after dec_end_kernel of frame f): what
// dec_output_kernel does for I420 -- got, and the picture pic[outpar] cropped by its SPS, read where it
// lies (coded strides, crop origin) and written as tight RGBA8 into in[s].out. Grid (blocks, S).
__global__ __launch_bounds__(256) void dec_output_rgba_kernel(DecOutLaunch a) {
    const int s = blockIdx.y;
    if (s >= a.S) return;
    const DecState *st = a.desc[s].st;
    const DecInput &I = a.in[s];
    const int ok = st->got_pic && !st->err;
    if (I.got && blockIdx.x == 0 && threadIdx.x == 0) *I.got = ok;
    if (!ok || !I.out) return;
    const int c0 = st->ps.crop[0], c1 = st->ps.crop[1], c2 = st->ps.crop[2], c3 = st->ps.crop[3];
    const int W = a.cw - 2 * (c0 + c1), H = a.ch - 2 * (c2 + c3), x0 = 2 * c0, y0 = 2 * c2;
    if (W <= 0 || H <= 0) return;
    const uint8_t *const *pic = a.desc[s].pic[st->outpar & 1];
    const int ys = a.cw, uvs = a.cw / 2;
    i420_to_rgba_picture(pic[0] + (size_t)y0 * ys + x0, pic[1] + (size_t)(y0 / 2) * uvs + x0 / 2, pic[2] + (size_t)(y0 / 2) * uvs + x0 / 2,
                         ys, uvs, W, H, I.out, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// grid for n frames of w x h: every unit once when that is at most H264MI_COLOR_MAX_BLOCKS blocks
static dim3 color_grid(int w, int h, int n) {
    const int ny = std::min(n, H264MI_COLOR_MAX_FRAMES_Y);
    const long long units = (long long)((w + 7) / 8) * (h / 2);
    const long long bx = std::max(1LL, std::min((units + 255) / 256, (long long)(H264MI_COLOR_MAX_BLOCKS / ny)));
    return dim3((unsigned)bx, (unsigned)ny);
}
// arguments of a conversion call: even positive sizes whose unit count fits the kernels' int indices
static bool color_args_ok(int w, int h, int n) {
    return w > 0 && h > 0 && n > 0 && !(w & 1) && !(h & 1) && (long long)((w + 7) / 8) * (h / 2) < (1LL << 30);
}
// (each launch first drops whatever error an earlier, unrelated HIP call of the thread left behind -- an event
// query that was not ready, say -- so that what it returns is its own)
static int launch_rgba_to_i420(const uint8_t *d_rgba, int w, int h, int n, uint8_t *d_out, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(rgba_to_i420_kernel, color_grid(w, h, n), dim3(256), 0, s, d_rgba, d_out, w, h, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
static int launch_i420_to_rgba(const I420Pics &p, int w, int h, int n, uint8_t *d_rgba, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(i420_to_rgba_kernel, color_grid(w, h, n), dim3(256), 0, s, p, w, h, n, d_rgba);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// n tight I420 frames back to back
static I420Pics tight_i420(const uint8_t *d, int w, int h) {
    const size_t ysz = (size_t)w * h, csz = (size_t)(w / 2) * (h / 2);
    return I420Pics{d, d + ysz, d + ysz + csz, ysz + 2 * csz, w, w / 2};
}
}  // namespace h264mi
