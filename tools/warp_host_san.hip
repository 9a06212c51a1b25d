// warp_host_san.hip -- the host rules of the mesh warp (csrc/picture_host.h and the host half of csrc/warp.hip) run
// under AddressSanitizer and UBSan on the CPU. A program of its own: nothing is loaded into Python, no kernel is
// launched, no device is needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/warp_host_san.hip openh264-wasm_amd/csrc/warp.hip \
//         -o warp_host_san && ./warp_host_san
//
// It runs, with every frame and mesh in a heap block of exactly the size the call may touch:
//   * warp_ok one past every limit of every field; warp_args_ok on null pointers, sides at and past 2 and 8192, n < 1,
//     misaligned meshes, and a destination one byte into and one byte clear of the source and of shared and per-frame
//     meshes;
//   * the three builders at the smallest and largest destinations and every pitch, at their limits and one past each
//     (INT32 extremes of the coefficients, a denominator of 1 and of 0 at the last control point, the radial limits and
//     q at 2^24 and just above), a refused call leaving the block untouched;
//   * warp_frame_host on the shapes of tests/test_gpu_warp.py (2x2, 16x16, 18x34 -> 34x18, 130x66, 2x2 <-> 130x66,
//     8192x2 <-> 2x8192) x three pitches x both filters x both edge modes under an identity, a rotation, a 1/8 zoom out,
//     a random mesh and a mesh of INT32_MAX and INT32_MIN, against a second statement that forms the position in 64
//     bits with a floor division and sums the sixteen taps in one pass order per row;
//   * warp_tile_class on every tile of those cases: 0 or 1, and -1 one past the last tile and plane.
// Prints one line per group and "ok"; exits 1 at the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../openh264-wasm_amd/csrc/picture_host.h"

using namespace h264mi;

static int failures = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);        \
            failures++;                                                  \
        }                                                                \
    } while (0)

template <class T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n]); }  // exactly n: ASan guards both ends

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int64_t fdiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
static int clampi(int64_t v, int lo, int hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

// the second statement of one frame
static void second(uint8_t *dst, int dw, int dh, const uint8_t *src, int sw, int sh, const int32_t *mesh, const h264mi_warp &p) {
    const int g = p.grid_log2, G = 1 << g, mw = warp_mesh_side(dw, g);
    const int fill[3] = {p.fill_y, p.fill_u, p.fill_v};
    size_t so = 0, dof = 0;
    for (int pl = 0; pl < 3; pl++) {
        const int c = pl != 0, pw = sw >> c, ph = sh >> c, qw = dw >> c, qh = dh >> c;
        for (int oy = 0; oy < qh; oy++)
            for (int ox = 0; ox < qw; ox++) {
                const int u = c ? 4 * ox + 1 : 2 * ox, v = c ? 4 * oy + 1 : 2 * oy;
                const int cx = u / (2 * G), cy = v / (2 * G), fx = u % (2 * G), fy = v % (2 * G);
                int64_t L[2];
                for (int k = 0; k < 2; k++) {
                    int64_t pt[4];
                    for (int j = 0; j < 4; j++) pt[j] = clampi(mesh[2 * ((size_t)(cy + (j >> 1)) * mw + cx + (j & 1)) + k], -(1 << 18), 1 << 18);
                    const int64_t P = (int64_t)(2 * G - fx) * (2 * G - fy) * pt[0] + (int64_t)fx * (2 * G - fy) * pt[1] +
                                      (int64_t)(2 * G - fx) * fy * pt[2] + (int64_t)fx * fy * pt[3];
                    L[k] = c ? fdiv(P - 28 * G * G, 8 * G * G) : fdiv(P + 2 * G * G, 4 * G * G);
                }
                const int64_t ix = fdiv(L[0], 16), iy = fdiv(L[1], 16);
                int wx[4], wy[4];
                up_weights((int)(L[0] - 16 * ix), p.filter == H264MI_FILTER_BICUBIC, wx);
                up_weights((int)(L[1] - 16 * iy), p.filter == H264MI_FILTER_BICUBIC, wy);
                int64_t acc = 0;
                for (int t = 3; t >= 0; t--) {
                    int64_t h = 0;
                    for (int j = 3; j >= 0; j--) h += (int64_t)wx[j] * src[so + (size_t)clampi(iy - 1 + t, 0, ph - 1) * pw + clampi(ix - 1 + j, 0, pw - 1)];
                    acc += wy[t] * fdiv(h + 16, 32);
                }
                int o = clampi(fdiv(acc + (1 << 20), 1 << 21), 0, 255);
                if (p.edge == H264MI_WARP_FILL && (L[0] < 0 || L[0] > 16 * (pw - 1) || L[1] < 0 || L[1] > 16 * (ph - 1))) o = fill[pl];
                dst[dof + (size_t)oy * qw + ox] = (uint8_t)o;
            }
        so += (size_t)pw * ph;
        dof += (size_t)qw * qh;
    }
}

static void check_ok() {
    h264mi_warp good{1, 1, 255, 0, 128, 3};
    CHECK(warp_ok(&good) && !warp_ok(nullptr));
    for (int f = 0; f < 6; f++) {
        const int lo[6] = {0, 0, 0, 0, 0, 3}, hi[6] = {1, 1, 255, 255, 255, 5};
        for (int side = 0; side < 2; side++) {
            h264mi_warp w = good;
            int32_t fld[6];
            static_assert(sizeof(fld) == sizeof(w), "six int32_t fields");
            memcpy(fld, &w, sizeof(w));
            fld[f] = side ? hi[f] : lo[f];
            memcpy(&w, fld, sizeof(w));
            CHECK(warp_ok(&w));
            fld[f] = side ? hi[f] + 1 : lo[f] - 1;
            memcpy(&w, fld, sizeof(w));
            CHECK(!warp_ok(&w));
        }
    }
    // the pointers' values: nothing is dereferenced, so the addresses are made up
    const uintptr_t B = (uintptr_t)1 << 32;
    const int dw = 18, dh = 34, sw = 34, sh = 18, n = 3;
    const size_t db = n * i420_bytes(dw, dh), sb = n * i420_bytes(sw, sh), mb = warp_mesh_bytes(dw, dh, 3);
    uint8_t *src = (uint8_t *)B, *mesh = (uint8_t *)(B + ((uintptr_t)1 << 30)), *dst = (uint8_t *)(B + ((uintptr_t)2 << 30)), *far = (uint8_t *)(B + ((uintptr_t)3 << 30));
    CHECK(warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh, 1, &good) && warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh, 0, &good));
    CHECK(!warp_args_ok(nullptr, dw, dh, src, sw, sh, n, mesh, 1, &good) && !warp_args_ok(dst, dw, dh, nullptr, sw, sh, n, mesh, 1, &good));
    CHECK(!warp_args_ok(dst, dw, dh, src, sw, sh, n, nullptr, 1, &good) && !warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh, 1, nullptr));
    CHECK(!warp_args_ok(dst, dw, dh, src, sw, sh, 0, mesh, 1, &good) && !warp_args_ok(dst, dw, dh, src, sw, sh, -1, mesh, 1, &good));
    CHECK(!warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh, 2, &good) && !warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh, -1, &good));
    const int bad_side[] = {0, 1, -2, 3, 8193, 8194};
    for (int b : bad_side) {
        CHECK(!warp_args_ok(dst, b, dh, src, sw, sh, 1, mesh, 0, &good) && !warp_args_ok(dst, dw, b, src, sw, sh, 1, mesh, 0, &good));
        CHECK(!warp_args_ok(dst, dw, dh, src, b, sh, 1, mesh, 0, &good) && !warp_args_ok(dst, dw, dh, src, sw, b, 1, mesh, 0, &good));
    }
    CHECK(warp_args_ok(dst, 2, 2, src, 8192, 2, 1, mesh, 0, &good) && warp_args_ok(dst, 8192, 8192, src, 8192, 8192, 1, far, 0, &good));
    for (int off = 1; off < 4; off++) CHECK(!warp_args_ok(dst, dw, dh, src, sw, sh, n, mesh + off, 1, &good));
    CHECK(!warp_args_ok(src + sb - 1, dw, dh, src, sw, sh, n, mesh, 1, &good));   // the source's last byte
    CHECK(warp_args_ok(src + sb, dw, dh, src, sw, sh, n, mesh, 1, &good));
    CHECK(!warp_args_ok(src - db + 1, dw, dh, src, sw, sh, n, mesh, 1, &good));   // its first
    CHECK(warp_args_ok(src - db, dw, dh, src, sw, sh, n, mesh, 1, &good));
    CHECK(!warp_args_ok(mesh + n * mb - 1, dw, dh, src, sw, sh, n, mesh, 1, &good));  // the last mesh's last byte
    CHECK(warp_args_ok(mesh + n * mb, dw, dh, src, sw, sh, n, mesh, 1, &good));
    CHECK(warp_args_ok(mesh + mb, dw, dh, src, sw, sh, n, mesh, 0, &good));           // behind a shared mesh
    CHECK(!warp_args_ok(mesh + mb - 1, dw, dh, src, sw, sh, n, mesh, 0, &good));
    CHECK(!warp_args_ok(mesh - db + 1, dw, dh, src, sw, sh, n, mesh, 0, &good) && warp_args_ok(mesh - db, dw, dh, src, sw, sh, n, mesh, 0, &good));
    printf("checks: ok\n");
}

static void check_builders() {
    const int sizes[][2] = {{2, 2}, {16, 16}, {130, 66}, {8192, 2}, {2, 8192}, {8192, 8192}};
    for (auto &sz : sizes)
        for (int g = WARP_MIN_GRID; g <= WARP_MAX_GRID; g++) {
            const int dw = sz[0], dh = sz[1], mw = warp_mesh_side(dw, g), mh = warp_mesh_side(dh, g);
            const size_t words = 2 * (size_t)mw * mh;
            auto m = block<int32_t>(words);
            auto fill = [&] { for (size_t i = 0; i < words; i++) m[i] = 0x5A5A5A5A; };
            auto untouched = [&] { for (size_t i = 0; i < words; i++) if (m[i] != 0x5A5A5A5A) return false; return true; };
            auto inside = [&] { for (size_t i = 0; i < words; i++) if (m[i] < -WARP_POINT_MAX || m[i] > WARP_POINT_MAX) return false; return true; };
            const int32_t ident[6] = {65536, 0, 0, 0, 65536, 0}, big[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
            CHECK(warp_mesh_affine(m.get(), dw, dh, g, ident) == mw * mh && m[0] == 0 && m[2] == (16 << g) && m[2 * (size_t)mw + 1] == (16 << g));
            CHECK(warp_mesh_affine(m.get(), dw, dh, g, big) == mw * mh && inside());
            fill();
            CHECK(warp_mesh_affine(m.get(), dw, dh, 2, ident) == -1 && warp_mesh_affine(m.get(), dw, dh, 6, ident) == -1 &&
                  warp_mesh_affine(m.get(), dw + 1, dh, g, ident) == -1 && warp_mesh_affine(nullptr, dw, dh, g, ident) == -1 &&
                  warp_mesh_affine(m.get(), dw, dh, g, nullptr) == -1 && untouched());
            const int64_t X1 = (int64_t)(mw - 1) << g, Y1 = (int64_t)(mh - 1) << g;
            int32_t h[9] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, -1, -1, (int32_t)(X1 + Y1 + 1)};
            CHECK(warp_mesh_homography(m.get(), dw, dh, g, h) == mw * mh && inside());  // the last denominator is 1
            fill();
            h[8] -= 1;                                                                  // ... is 0
            CHECK(warp_mesh_homography(m.get(), dw, dh, g, h) == -1 && untouched());
            const int32_t hbig[9] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
            CHECK(warp_mesh_homography(m.get(), dw, dh, g, hbig) == mw * mh && inside());
            const int C = WARP_RADIAL_MAX_CENTRE, K = WARP_RADIAL_MAX_K;
            const int64_t R2 = WARP_RADIAL_MAX_R2;
            CHECK(warp_mesh_radial(m.get(), dw, dh, g, C, -C, R2, K, -K) == mw * mh && inside());
            CHECK(warp_mesh_radial(m.get(), dw, dh, g, -C, C, R2, -K, K) == mw * mh && inside());
            // q at its limit at the far corner: centre 0, so q = (X^2 + Y^2) 2^24 / r2 there, in sixteenths squared 2^8 more
            const int64_t far = ((X1 * X1 + Y1 * Y1) << 8) << 16;
            const int64_t r2_at = far / (WARP_RADIAL_MAX_Q + 1) + 1;  // the smallest r2 with q <= 2^24
            if (r2_at <= R2) CHECK(warp_mesh_radial(m.get(), dw, dh, g, 0, 0, r2_at, K, K) == mw * mh && inside());
            if (r2_at <= R2) CHECK(warp_mesh_radial(m.get(), dw, dh, g, 0, 0, r2_at, -K, -K) == mw * mh && inside());
            fill();
            if (r2_at > 1 && r2_at - 1 <= R2) CHECK(warp_mesh_radial(m.get(), dw, dh, g, 0, 0, r2_at - 1, K, K) == -1);
            CHECK(warp_mesh_radial(m.get(), dw, dh, g, C + 1, 0, R2, 0, 0) == -1 && warp_mesh_radial(m.get(), dw, dh, g, 0, -C - 1, R2, 0, 0) == -1 &&
                  warp_mesh_radial(m.get(), dw, dh, g, 0, 0, R2 + 1, 0, 0) == -1 && warp_mesh_radial(m.get(), dw, dh, g, 0, 0, 0, 0, 0) == -1 &&
                  warp_mesh_radial(m.get(), dw, dh, g, 0, 0, R2, K + 1, 0) == -1 && warp_mesh_radial(m.get(), dw, dh, g, 0, 0, R2, 0, -K - 1) == -1 &&
                  warp_mesh_radial(m.get(), dw, dh, g, 0, 0, INT64_MIN, 0, 0) == -1 && warp_mesh_radial(m.get(), dw, dh, g, 0, 0, INT64_MAX, 0, 0) == -1 &&
                  untouched());
        }
    printf("builders: ok\n");
}

static void check_frames() {
    const int shapes[][4] = {{2, 2, 2, 2}, {16, 16, 16, 16}, {18, 34, 34, 18}, {130, 66, 130, 66}, {2, 2, 130, 66}, {130, 66, 2, 2},
                             {8192, 2, 2, 8192}, {2, 8192, 8192, 2}};
    long frames = 0, tiles = 0;
    for (auto &s : shapes)
        for (int g = WARP_MIN_GRID; g <= WARP_MAX_GRID; g++) {
            const int sw = s[0], sh = s[1], dw = s[2], dh = s[3], mw = warp_mesh_side(dw, g), mh = warp_mesh_side(dh, g);
            const size_t sb = i420_bytes(sw, sh), db = i420_bytes(dw, dh), words = 2 * (size_t)mw * mh;
            auto src = block<uint8_t>(sb);
            auto a = block<uint8_t>(db);
            auto b = block<uint8_t>(db);
            auto m = block<int32_t>(words);
            for (size_t i = 0; i < sb; i++) src[i] = (uint8_t)rnd();
            for (int kind = 0; kind < 5; kind++) {
                const int32_t ident[6] = {65536, 0, 0, 0, 65536, 0}, rot[6] = {65048, -7987, 4 << 16, 7987, 65048, -(3 << 16)},
                              out8[6] = {8 << 16, 0, -98304, 0, 8 << 16, 16384};
                if (kind < 3) CHECK(warp_mesh_affine(m.get(), dw, dh, g, kind == 0 ? ident : kind == 1 ? rot : out8) == mw * mh);
                if (kind == 3) for (size_t i = 0; i < words; i++) m[i] = (int32_t)(rnd() % (16 * (uint32_t)((i & 1) ? sh : sw) + 128)) - 64;
                if (kind == 4) for (size_t i = 0; i < words; i++) m[i] = (rnd() & 1) ? INT32_MAX : INT32_MIN;
                for (int filter = 0; filter < 2; filter++)
                    for (int edge = 0; edge < 2; edge++) {
                        const h264mi_warp p{filter, edge, 31, 77, 201, g};
                        warp_frame_host(a.get(), dw, dh, src.get(), sw, sh, m.get(), p);
                        second(b.get(), dw, dh, src.get(), sw, sh, m.get(), p);
                        CHECK(memcmp(a.get(), b.get(), db) == 0);
                        if (kind == 0 && sw == dw && sh == dh) CHECK(memcmp(a.get(), src.get(), db) == 0);
                        frames++;
                    }
                for (int pl = 0; pl < 3; pl++)
                    for (int ty = 0; ty < mh - 1; ty++)
                        for (int tx = 0; tx < mw - 1; tx++) {
                            const int c = warp_tile_class(m.get(), dw, dh, sw, sh, g, pl, tx, ty);
                            CHECK(c == 0 || c == 1);
                            tiles++;
                        }
                CHECK(warp_tile_class(m.get(), dw, dh, sw, sh, g, 3, 0, 0) == -1 && warp_tile_class(m.get(), dw, dh, sw, sh, g, 0, mw - 1, 0) == -1 &&
                      warp_tile_class(m.get(), dw, dh, sw, sh, g, 0, 0, mh - 1) == -1 && warp_tile_class(m.get(), dw, dh, sw, sh, g, -1, 0, 0) == -1 &&
                      warp_tile_class(nullptr, dw, dh, sw, sh, g, 0, 0, 0) == -1);
            }
        }
    printf("frames: %ld against the second statement, %ld tile classes: ok\n", frames, tiles);
}

int main() {
    check_ok();
    check_builders();
    check_frames();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
