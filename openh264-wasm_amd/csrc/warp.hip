// warp.hip -- tight I420 frames resampled along a control-point mesh on the device (gfx950), as include/h264mi.h
// defines it (h264mi_i420_warp_dev, h264mi_enc_encode_warped, the h264mi_warp_mesh_* builders). DESIGN.md §5.20.
//   warp_kernel : n frames per launch -- the standalone call, or an encoder's source frames warped into its input area
// The rule in short (the header has it in full). A mesh holds a source luma position, in sixteenths of a sample, for
// every G = 1 << grid_log2 destination luma samples each way. An output sample sits at (u, v) of a doubled grid (luma
// 2 ox, chroma 4 cx + 1), which names a cell and two fractions; the cell's four points are blended by the fractions
// with integer weights that sum to 4 G^2 (warp_pos), which gives the source position L of the sample's own plane in
// sixteenths; i = L >> 4 and f = L & 15 select the taps i - 1 .. i + 2 per axis, clamped to the plane, and the phase
// of up_weights; the two passes round as upscale.hip's do. int32 throughout: a point is clamped to +-2^18 as it is
// read, so |P| <= 4 G^2 2^18 = 2^30.
//
// Work split. The destination side is regular, the source side is a gather. A wave owns one tile: the samples of one
// mesh cell in one plane of one frame (G x G luma samples, G/2 x G/2 chroma samples; fewer at the right and lower
// edge). The item index, hence the cell and its four control points, is the same in every lane: the points are
// fetched by scalar loads and the blend's corner weights are the only per-lane part of a position. The lanes lie
// row-major over the tile, T = 4, 8, 16 or 32 columns by 64 / T rows at a time, so four consecutive lanes hold four
// consecutive samples of a destination row and picture_dev.h's segment store writes them as a dword where the row's
// first address allows it. A chroma tile at grid_log2 3 is 4 x 4 samples and fills a quarter of the wave; measured
// (profiles/warp/warp_ab.md, a 7-degree rotation of 1080p frames) pitch 8 takes 2.7 times as long as pitch 16, pitch 32 0.6 times.
// The gather. A position is bilinear in the fractions, so over a tile it takes its extremes at the tile's four corner
// samples: the bounding box of those four positions, widened by the tap margin (one before, two after) and clamped to
// the plane, holds every tap of the tile (warp_tile_box), and it is known before a sample is read. Two classes
// (warp_box_staged, a pure function of the control points and the geometry):
//   staged   : the box has at most H264MI_WARP_BOX_BYTES samples. The wave copies it to its own 2 KB of LDS with row-wise
//              loads -- consecutive lanes read consecutive bytes of a box row -- and every tap is a ds_read_u8.
//              Measured on that rotation: 1.19x faster than the fallback with bicubic taps, 0.84x with bilinear.
//              Identity, shifts, rotations, lens corrections and enlargements are in this class at every pitch.
//   fallback : anything larger (a mesh that shrinks by more than about 1.3 at pitch 32, more at the finer pitches; a
//              folded or random mesh). Every tap is a clamped byte load from global memory.
// Both read the same samples under the same arithmetic (warp_sample is one template over the fetch), so they give the
// same bytes. The four waves of a block take four consecutive items and step together, so the two barriers around the
// LDS image are uniform; a wave past the last item computes the last item again and stores nothing.
// Nothing is read outside the source planes -- every tap index is clamped to 0 .. p - 1 before it is used, in both
// classes, and the box is a sub-rectangle of the plane -- and nothing is written outside the destination planes: a lane
// stores only inside its tile's nx x ny samples. No atomics, no device allocation, no host-to-device copy.
//
// A translation unit and a code object of its own, as the other picture units are. The host runtime (capi_enc.inc)
// reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <stdint.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define H264MI_WARP_BOX_BYTES 2048        // a wave's LDS image: the largest staged box
#define H264MI_WARP_MAX_ITEMS (1 << 30)   // tiles in one launch

struct WarpLaunch {
    const uint8_t *src;
    uint8_t *dst;
    const int32_t *mesh;
    size_t sfb, dfb, mstride;  // frame f: src + f * sfb, dst + f * dfb, mesh + f * mstride words (0: one mesh for all)
    int sw, sh, dw, dh;
    int g, mw;                 // grid_log2; control points across
    int ntx, nty, n;           // tiles across and down a plane (the same for luma and chroma); frames
    int cubic, fill_on, fill[3];
    int path;                  // 0: the class decides; 1: every tile takes the fallback (measurement)
};

struct WarpCell { int x[4], y[4]; };     // the cell's points A (top left), B (top right), C, D, clamped
struct WarpBox { int x0, y0, w, h; };    // a sub-rectangle of the source plane

__host__ __device__ static inline int warp_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// a control point's coordinate as it is used
__host__ __device__ static inline int warp_point(int32_t v) { return warp_clampi(v, -WARP_POINT_MAX, WARP_POINT_MAX); }
// the cell (cx, cy) of a mesh of mw points across
__host__ __device__ static inline WarpCell warp_cell(const int32_t *mesh, int mw, int cx, int cy) {
    const int32_t *r0 = mesh + 2 * ((size_t)cy * mw + cx), *r1 = r0 + 2 * (size_t)mw;
    WarpCell k;
    k.x[0] = warp_point(r0[0]); k.y[0] = warp_point(r0[1]); k.x[1] = warp_point(r0[2]); k.y[1] = warp_point(r0[3]);
    k.x[2] = warp_point(r1[0]); k.y[2] = warp_point(r1[1]); k.x[3] = warp_point(r1[2]); k.y[3] = warp_point(r1[3]);
    return k;
}
// L of one coordinate: the four points c[] blended at the fractions fx, fy (0 .. 2G - 1 of the doubled grid), as a
// position in sixteenths of the plane's own samples. The weights are non-negative and sum to 4 G^2 <= 4096, the
// points are within +-2^18: every partial sum is within +-2^30
__host__ __device__ static inline int warp_pos(const int *c, int fx, int fy, int g, bool chroma) {
    const int G2 = 2 << g, GG = 1 << (2 * g);
    const int P = (G2 - fx) * (G2 - fy) * c[0] + fx * (G2 - fy) * c[1] + (G2 - fx) * fy * c[2] + fx * fy * c[3];
    return chroma ? (P - 28 * GG) >> (2 * g + 3) : (P + 2 * GG) >> (2 * g + 2);
}
// the fraction of sample j of a tile, per axis: u = 2 o (luma) or 4 o + 1 (chroma) below the cell's 2 G
__host__ __device__ static inline int warp_frac(int j, bool chroma) { return chroma ? 4 * j + 1 : 2 * j; }
// the source box of a tile of nx x ny samples (from the cell's first sample on) of a pw x ph source plane: the
// positions of the four corner samples bound every sample's, being bilinear between them
__host__ __device__ static inline WarpBox warp_tile_box(const WarpCell &k, int g, bool chroma, int nx, int ny, int pw, int ph) {
    const int fx[2] = {warp_frac(0, chroma), warp_frac(nx - 1, chroma)}, fy[2] = {warp_frac(0, chroma), warp_frac(ny - 1, chroma)};
    int lx0 = INT32_MAX, lx1 = INT32_MIN, ly0 = INT32_MAX, ly1 = INT32_MIN;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const int lx = warp_pos(k.x, fx[a], fy[b], g, chroma), ly = warp_pos(k.y, fx[a], fy[b], g, chroma);
            lx0 = lx < lx0 ? lx : lx0; lx1 = lx > lx1 ? lx : lx1;
            ly0 = ly < ly0 ? ly : ly0; ly1 = ly > ly1 ? ly : ly1;
        }
    WarpBox b;
    b.x0 = warp_clampi((lx0 >> 4) - 1, 0, pw - 1);
    b.y0 = warp_clampi((ly0 >> 4) - 1, 0, ph - 1);
    b.w = warp_clampi((lx1 >> 4) + 2, 0, pw - 1) - b.x0 + 1;
    b.h = warp_clampi((ly1 >> 4) + 2, 0, ph - 1) - b.y0 + 1;
    return b;
}
// the class of a tile: sides are at most 8192, the product stays in 32 bits
__host__ __device__ static inline bool warp_box_staged(const WarpBox &b) { return b.w * b.h <= H264MI_WARP_BOX_BYTES; }

// the fetch of a sample (x, y) of the source plane, both inside it: from the wave's LDS image of the box, or from memory
struct WarpFromLds {
    const uint8_t *img; int x0, y0, w;
    PICDEV int operator()(int x, int y) const { return img[(y - y0) * w + (x - x0)]; }
};
struct WarpFromMem {
    const uint8_t *S; int pw;
    PICDEV int operator()(int x, int y) const { return S[(size_t)y * pw + x]; }
};
// the sample at the position (lx, ly) of a pw x ph plane: the taps clamped, horizontal first, the upscaler's rounding
template <class Fetch>
PICDEV uint32_t warp_sample(const Fetch &px, int lx, int ly, int pw, int ph, bool cubic) {
    const int ix = lx >> 4, iy = ly >> 4;
    int wx[4], wy[4], xi[4], yi[4];
    up_weights(lx & 15, cubic, wx);
    up_weights(ly & 15, cubic, wy);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        xi[t] = warp_clampi(ix - 1 + t, 0, pw - 1);
        yi[t] = warp_clampi(iy - 1 + t, 0, ph - 1);
    }
    int acc = 0;
    if (cubic) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int h = wx[0] * px(xi[0], yi[t]) + wx[1] * px(xi[1], yi[t]) + wx[2] * px(xi[2], yi[t]) + wx[3] * px(xi[3], yi[t]);
            acc += wy[t] * ((h + 16) >> 5);
        }
    } else {  // the outer weights are 0: their taps are not read
#pragma unroll
        for (int t = 1; t < 3; t++) {
            const int h = wx[1] * px(xi[1], yi[t]) + wx[2] * px(xi[2], yi[t]);
            acc += wy[t] * ((h + 16) >> 5);
        }
    }
    return (uint32_t)warp_clampi((acc + (1 << 20)) >> 21, 0, 255);
}

// what a wave knows about its tile, the same in every lane
struct WarpTile {
    const uint8_t *S; uint8_t *D;
    WarpCell k;
    int pw, ph, qw, x0, y0, nx, ny, lt, fill;
    bool chroma;
};
// the tile's samples, 64 at a time: lane -> column lane & (T - 1), row lane >> lt of the pass
template <class Fetch>
PICDEV void warp_tile(const WarpTile &t, const Fetch &px, int g, bool cubic, bool fill_on, bool live, int lane) {
    const int T = 1 << t.lt, rows = 64 >> t.lt;
    const int c = lane & (T - 1), r0 = lane >> t.lt;
    const int fx = warp_frac(min(c, t.nx - 1), t.chroma);  // a lane beyond the tile computes its last column or row
    for (int rb = 0; rb < t.ny; rb += rows) {
        const int r = rb + r0;
        const int fy = warp_frac(min(r, t.ny - 1), t.chroma);
        const int lx = warp_pos(t.k.x, fx, fy, g, t.chroma), ly = warp_pos(t.k.y, fx, fy, g, t.chroma);
        uint32_t v = warp_sample(px, lx, ly, t.pw, t.ph, cubic);
        if (fill_on && (lx < 0 || lx > 16 * (t.pw - 1) || ly < 0 || ly > 16 * (t.ph - 1))) v = (uint32_t)t.fill;
        const uint32_t q = seg_pack(v);  // every lane runs it
        if (live && r < t.ny) seg_store(t.D + (size_t)(t.y0 + r) * t.qw + t.x0, c, t.nx, v, q);
    }
}

__global__ __launch_bounds__(256) void warp_kernel(WarpLaunch a) {
    __shared__ uint8_t lds[4][H264MI_WARP_BOX_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: what follows from it is per wave
    const int ntt = a.ntx * a.nty, per = 3 * ntt, items = per * a.n;            // at most 2^30 (launch_warp_i420)
    const bool cubic = a.cubic != 0, fill_on = a.fill_on != 0;
    for (int base = (int)blockIdx.x * 4; base < items; base += (int)gridDim.x * 4) {  // the same count in every wave of a block
        const bool live = base + wave < items;
        const int it = min(base + wave, items - 1);
        const int f = it / per;
        int k = it - f * per;
        const int p = k / ntt;
        k -= p * ntt;
        const int ty = k / a.ntx, tx = k - ty * a.ntx;
        const int sh1 = p != 0;  // chroma: every size halved
        WarpTile t;
        t.chroma = sh1 != 0;
        t.pw = a.sw >> sh1; t.ph = a.sh >> sh1; t.qw = a.dw >> sh1;
        const int qh = a.dh >> sh1;
        t.lt = a.g - sh1;
        t.x0 = tx << t.lt; t.y0 = ty << t.lt;
        t.nx = min(1 << t.lt, t.qw - t.x0); t.ny = min(1 << t.lt, qh - t.y0);  // both at least 1: ntx = ceil(dw / G)
        t.fill = p == 0 ? a.fill[0] : p == 1 ? a.fill[1] : a.fill[2];
        const size_t sy_b = (size_t)a.sw * a.sh, sc_b = (size_t)(a.sw >> 1) * (a.sh >> 1);
        const size_t dy_b = (size_t)a.dw * a.dh, dc_b = (size_t)(a.dw >> 1) * (a.dh >> 1);
        t.S = a.src + (size_t)f * a.sfb + (p == 0 ? 0 : p == 1 ? sy_b : sy_b + sc_b);
        t.D = a.dst + (size_t)f * a.dfb + (p == 0 ? 0 : p == 1 ? dy_b : dy_b + dc_b);
        t.k = warp_cell(a.mesh + (size_t)f * a.mstride, a.mw, tx, ty);
        const WarpBox b = warp_tile_box(t.k, a.g, t.chroma, t.nx, t.ny, t.pw, t.ph);
        const bool staged = a.path == 0 && warp_box_staged(b);
        uint8_t *img = lds[wave];
        if (staged) {  // box rows back to back; consecutive lanes read consecutive bytes of a row
            const int nb = b.w * b.h;
            for (int i = lane; i < nb; i += 64) {
                const int r = (int)((uint32_t)i / (uint32_t)b.w), c = i - r * b.w;
                img[i] = t.S[(size_t)(b.y0 + r) * t.pw + b.x0 + c];
            }
        }
        __syncthreads();
        if (staged) warp_tile(t, WarpFromLds{img, b.x0, b.y0, b.w}, a.g, cubic, fill_on, live, lane);
        else warp_tile(t, WarpFromMem{t.S, t.pw}, a.g, cubic, fill_on, live, lane);
        __syncthreads();  // the image is free for the next item
    }
}

// ---- host
// n tight sw x sh I420 frames at src to n tight dw x dh frames at dst along the mesh(es) at mesh; arguments as
// warp_args_ok accepts them. As many frames to a launch as keep its tile count within 2^30. path 0: the class of a tile
// decides how it reads; path 1 (tools/warp_ab.py only): every tile samples global memory
int launch_warp_i420(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, int n, const int32_t *mesh, int mesh_per_frame,
                     const h264mi_warp &p, int path, hipStream_t s) {
    WarpLaunch a{};
    a.sfb = i420_bytes(sw, sh); a.dfb = i420_bytes(dw, dh);
    a.sw = sw; a.sh = sh; a.dw = dw; a.dh = dh;
    a.g = p.grid_log2;
    a.mw = warp_mesh_side(dw, p.grid_log2);
    a.mstride = mesh_per_frame ? (size_t)a.mw * warp_mesh_side(dh, p.grid_log2) * 2 : 0;
    a.ntx = a.mw - 1; a.nty = warp_mesh_side(dh, p.grid_log2) - 1;
    a.cubic = p.filter == H264MI_FILTER_BICUBIC;
    a.fill_on = p.edge == H264MI_WARP_FILL;
    a.fill[0] = p.fill_y; a.fill[1] = p.fill_u; a.fill[2] = p.fill_v;
    a.path = path == 1 ? 1 : 0;
    const int per = 3 * a.ntx * a.nty;  // at most 3 * 1024 * 1024
    const int chunk = H264MI_WARP_MAX_ITEMS / per;
    (void)hipGetLastError();
    for (int f0 = 0; f0 < n; f0 += chunk) {
        a.n = std::min(n - f0, chunk);
        a.src = src + (size_t)f0 * a.sfb;
        a.dst = dst + (size_t)f0 * a.dfb;
        a.mesh = mesh + (size_t)f0 * a.mstride;
        hipLaunchKernelGGL(warp_kernel, dim3(launch_blocks((long long)per * a.n)), dim3(256), 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the definition on the host, one frame: every sample from its own (u, v), no tiles
void warp_frame_host(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, const int32_t *mesh, const h264mi_warp &p) {
    const int g = p.grid_log2, mw = warp_mesh_side(dw, g);
    const bool cubic = p.filter == H264MI_FILTER_BICUBIC;
    const int fill[3] = {p.fill_y, p.fill_u, p.fill_v};
    const uint8_t *S = src;
    uint8_t *D = dst;
    for (int pl = 0; pl < 3; pl++) {
        const int sh1 = pl != 0, pw = sw >> sh1, ph = sh >> sh1, qw = dw >> sh1, qh = dh >> sh1;
        for (int oy = 0; oy < qh; oy++)
            for (int ox = 0; ox < qw; ox++) {
                const int u = sh1 ? 4 * ox + 1 : 2 * ox, v = sh1 ? 4 * oy + 1 : 2 * oy;
                const WarpCell k = warp_cell(mesh, mw, u >> (g + 1), v >> (g + 1));
                const int fx = u & ((2 << g) - 1), fy = v & ((2 << g) - 1);
                const int lx = warp_pos(k.x, fx, fy, g, sh1 != 0), ly = warp_pos(k.y, fx, fy, g, sh1 != 0);
                const int ix = lx >> 4, iy = ly >> 4;
                int wx[4], wy[4], acc = 0;
                up_weights(lx & 15, cubic, wx);
                up_weights(ly & 15, cubic, wy);
                for (int t = 0; t < 4; t++) {
                    const uint8_t *row = S + (size_t)warp_clampi(iy - 1 + t, 0, ph - 1) * pw;
                    int h = 0;
                    for (int j = 0; j < 4; j++) h += wx[j] * row[warp_clampi(ix - 1 + j, 0, pw - 1)];
                    acc += wy[t] * ((h + 16) >> 5);
                }
                int o = warp_clampi((acc + (1 << 20)) >> 21, 0, 255);
                if (p.edge == H264MI_WARP_FILL && (lx < 0 || lx > 16 * (pw - 1) || ly < 0 || ly > 16 * (ph - 1))) o = fill[pl];
                D[(size_t)oy * qw + ox] = (uint8_t)o;
            }
        S += (size_t)pw * ph;
        D += (size_t)qw * qh;
    }
}

int warp_tile_class(const int32_t *mesh, int dw, int dh, int sw, int sh, int grid_log2, int plane, int tx, int ty) {
    if (!mesh || !canvas_ok(dw, dh) || !canvas_ok(sw, sh) || !warp_grid_ok(grid_log2) || plane < 0 || plane > 2) return -1;
    const int mw = warp_mesh_side(dw, grid_log2), mh = warp_mesh_side(dh, grid_log2);
    if (tx < 0 || ty < 0 || tx >= mw - 1 || ty >= mh - 1) return -1;
    const int sh1 = plane != 0, lt = grid_log2 - sh1;
    const int nx = std::min(1 << lt, (dw >> sh1) - (tx << lt)), ny = std::min(1 << lt, (dh >> sh1) - (ty << lt));
    return warp_box_staged(warp_tile_box(warp_cell(mesh, mw, tx, ty), grid_log2, sh1 != 0, nx, ny, sw >> sh1, sh >> sh1)) ? 0 : 1;
}

// ---- the builders (host only, integers only; the header states each rule)
static inline int64_t floor_div64(int64_t a, int64_t b) {  // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
static inline int32_t warp_clamp64(int64_t v) { return (int32_t)(v < -WARP_POINT_MAX ? -WARP_POINT_MAX : v > WARP_POINT_MAX ? WARP_POINT_MAX : v); }
static bool mesh_args_ok(const int32_t *mesh, int dw, int dh, int grid_log2) { return mesh && canvas_ok(dw, dh) && warp_grid_ok(grid_log2); }

int warp_mesh_affine(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t *m) {
    if (!mesh_args_ok(mesh, dw, dh, grid_log2) || !m) return -1;
    const int mw = warp_mesh_side(dw, grid_log2), mh = warp_mesh_side(dh, grid_log2);
    for (int j = 0; j < mh; j++)
        for (int i = 0; i < mw; i++) {
            const int64_t X = (int64_t)i << grid_log2, Y = (int64_t)j << grid_log2;  // |m X| < 2^31 * 2^14
            int32_t *pt = mesh + 2 * ((size_t)j * mw + i);
            pt[0] = warp_clamp64((m[0] * X + m[1] * Y + m[2] + (1 << 11)) >> 12);
            pt[1] = warp_clamp64((m[3] * X + m[4] * Y + m[5] + (1 << 11)) >> 12);
        }
    return mw * mh;
}
int warp_mesh_homography(int32_t *mesh, int dw, int dh, int grid_log2, const int32_t *h) {
    if (!mesh_args_ok(mesh, dw, dh, grid_log2) || !h) return -1;
    const int mw = warp_mesh_side(dw, grid_log2), mh = warp_mesh_side(dh, grid_log2);
    for (int pass = 0; pass < 2; pass++)  // the denominators first: a refusal writes nothing
        for (int j = 0; j < mh; j++)
            for (int i = 0; i < mw; i++) {
                const int64_t X = (int64_t)i << grid_log2, Y = (int64_t)j << grid_log2;
                const int64_t den = h[6] * X + h[7] * Y + h[8];  // every sum below 3 * 2^45; 32 num + den below 2^53
                if (pass == 0) {
                    if (den <= 0) return -1;
                    continue;
                }
                int32_t *pt = mesh + 2 * ((size_t)j * mw + i);
                pt[0] = warp_clamp64(floor_div64(32 * (h[0] * X + h[1] * Y + h[2]) + den, 2 * den));
                pt[1] = warp_clamp64(floor_div64(32 * (h[3] * X + h[4] * Y + h[5]) + den, 2 * den));
            }
    return mw * mh;
}
// |centre| <= 2^18 and X <= 16 * 8224 give |d| < 2^19, d^2 + d^2 < 2^39, << 16 below 2^55. q <= 2^24 (refused beyond)
// and |k| <= 2^20 give |k1 q| <= 2^44, q q <= 2^48, |k2 (q q >> 16)| <= 2^52, |s| < 2^37 and |d s| < 2^56
int warp_mesh_radial(int32_t *mesh, int dw, int dh, int grid_log2, int cx, int cy, int64_t r2, int k1, int k2) {
    if (!mesh_args_ok(mesh, dw, dh, grid_log2)) return -1;
    if (cx < -WARP_RADIAL_MAX_CENTRE || cx > WARP_RADIAL_MAX_CENTRE || cy < -WARP_RADIAL_MAX_CENTRE || cy > WARP_RADIAL_MAX_CENTRE) return -1;
    if (r2 < 1 || r2 > WARP_RADIAL_MAX_R2 || k1 < -WARP_RADIAL_MAX_K || k1 > WARP_RADIAL_MAX_K || k2 < -WARP_RADIAL_MAX_K || k2 > WARP_RADIAL_MAX_K)
        return -1;
    const int mw = warp_mesh_side(dw, grid_log2), mh = warp_mesh_side(dh, grid_log2);
    for (int pass = 0; pass < 2; pass++)  // every q first: a refusal writes nothing
        for (int j = 0; j < mh; j++)
            for (int i = 0; i < mw; i++) {
                const int64_t dx = (((int64_t)i << grid_log2) << 4) - cx, dy = (((int64_t)j << grid_log2) << 4) - cy;
                const int64_t q = ((dx * dx + dy * dy) << 16) / r2;
                if (pass == 0) {
                    if (q > WARP_RADIAL_MAX_Q) return -1;
                    continue;
                }
                const int64_t s = 65536 + ((k1 * q) >> 16) + ((k2 * ((q * q) >> 16)) >> 16);
                int32_t *pt = mesh + 2 * ((size_t)j * mw + i);
                pt[0] = warp_clamp64(cx + ((dx * s + (1 << 15)) >> 16));
                pt[1] = warp_clamp64(cy + ((dy * s + (1 << 15)) >> 16));
            }
    return mw * mh;
}
}  // namespace h264mi
