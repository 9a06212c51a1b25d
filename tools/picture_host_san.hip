// picture_host_san.hip -- the host rules of the picture calls (csrc/picture_host.h and the host halves of scale.hip,
// compose.hip, overlay.hip, upscale.hip, orient.hip, denoise.hip, scenecut.hip, deinterlace.hip, spatial.hip, levels.hip) run under AddressSanitizer and UBSan on the CPU. A program of its own: nothing
// is loaded into Python, no kernel is launched, no device is needed.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/picture_host_san.hip openh264-wasm_amd/csrc/scale.hip \
//         openh264-wasm_amd/csrc/compose.hip openh264-wasm_amd/csrc/overlay.hip openh264-wasm_amd/csrc/upscale.hip \
//         openh264-wasm_amd/csrc/orient.hip openh264-wasm_amd/csrc/denoise.hip openh264-wasm_amd/csrc/scenecut.hip \
//         openh264-wasm_amd/csrc/deinterlace.hip openh264-wasm_amd/csrc/spatial.hip openh264-wasm_amd/csrc/levels.hip \
//         -o picture_host_san && ./picture_host_san
//
// It runs, with every table in a heap block of exactly the size the call may touch:
//   * cells_ok (both values of may_enlarge) on valid lists and on every field of a cell made odd, negative, one past the
//     source or canvas, running over the edge, and larger than the crop on one axis and on both; on two cells touching,
//     sharing one sample, and on different canvases; on null and out-of-range counts -- each verdict against a
//     restatement in 64-bit arithmetic;
//   * fill_cell_table and the 64-to-a-launch split on lists of 1, 64, 65 and 4096 cells, cell_kind's split of a mixed
//     list, and overlay_launch_end on disjoint and on stacked placements of the same lengths;
//   * mosaic_cells and speaker_cells for 1, 64, 65 and 4096 sources and the sizes of tests/test_compose_host.py, their
//     cells checked by cells_ok, and their refusals;
//   * the scalar checks (scale, upscale, fill, overlay, sprite conversion) at their limits, the byte counts and the
//     range test;
//   * orient.hip's host restatement of a turned plane against the header's table, compose and inverse against planes
//     turned twice, its sizes and scalar check at their limits.
//   * the pixel-layout rules (pix_span, pix_layout_ok, pix_layout_tight, pix_ranges_overlap): every verdict and span
//     against a restatement in 128-bit arithmetic over random fields and extreme ones (INT32_MAX pitches, INT64_MAX
//     offsets and strides, negative values), and the tight layouts and spans of the five formats against their byte counts.
//   * the same for the formats 16..24 (I422 .. V210) with the unit rule -- every used pitch, offset, frame_stride and the
//     base a multiple of 1, 2 or 4 --, V210's tight pitch, ids 5..15 and 25 refused, pix_unit, and pixopt_ok at and past
//     its limits.
//   * denoise.hip's host restatement denoise_frame_host on heap blocks of exactly the frame's bytes at seven sizes (2x2
//     and partial blocks among them), out of place and in place, against a per-sample restatement; the k tables at the
//     limits of the parameters; denoise_ok and denoise_args_ok at their limits and one past each.
//   * scenecut.hip's host restatement scenecut_frame_host on heap blocks of exactly the frame's and the thumbnail's bytes
//     at seven sizes (cells 2 wide and high, partial blocks, more than one strip and block row), with and without each
//     output and in place, against a per-cell restatement; the cut test at its boundary; scenecut_ok and
//     scenecut_args_ok at their limits and one past each.
//   * deinterlace.hip's host restatement deinterlace_frame_host on heap blocks of exactly the frame's bytes at eight
//     sizes (2x2, one-row and five-row chroma planes, more than one strip and row group), for every parity x spatial x
//     temporal, with and without a previous frame, out of place and in place, against a second per-sample loop that
//     walks the scores in another order; deinterlace_ok and deinterlace_args_ok at their limits and one past each.
//   * spatial.hip's host restatements spatial_frame_host and privacy_frames_host on heap blocks of exactly the frames'
//     bytes: the filter at seven sizes (2x2, planes narrower than the stencil, more than one tile both ways) x eight
//     parameter sets against a restatement that sums columns first and floors without a shift, the masks of three lists
//     on three frames against a per-sample restatement; spatial_ok, spatial_args_ok and privacy_ok at their limits and
//     one past each, lists of 4096 entries and one more.
//   * levels.hip's host restatements hist_frame_host, lut_frame_host and levels_lut_host on heap blocks of exactly the
//     frame's, the histogram's, the tables', the state's and the record's bytes at six sizes x three contents x eight
//     parameter sets, without a state, as a first and as a later frame, against a second statement (counts from sorted
//     samples, sums taken afresh in 64 bits, the division as a search); levels_ok one past every limit, the clip counts
//     at the limits, hist_args_ok, lut_args_ok and levels_args_ok at the edges of every overlap and alignment rule.
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

// a list in a heap block of exactly n cells, so that a read past the end is the sanitizer's to see
static std::unique_ptr<h264mi_cell[]> heap(const std::vector<h264mi_cell> &v) {
    std::unique_ptr<h264mi_cell[]> p(new h264mi_cell[v.size()]);
    for (size_t k = 0; k < v.size(); k++) p[k] = v[k];
    return p;
}

// the rules of include/h264mi.h restated: 64-bit, one predicate per rule
static bool ref_ok(long long cw, long long ch, long long ncanvas, long long sw, long long sh, long long nsrc, const std::vector<h264mi_cell> &cells,
                   bool may_enlarge) {
    auto even_in = [](long long v, long long lo, long long hi) { return v % 2 == 0 && v >= lo && v <= hi; };
    if (ncanvas < 1 || nsrc < 1 || cells.empty() || cells.size() > 4096) return false;
    if (!even_in(cw, 2, 8192) || !even_in(ch, 2, 8192) || !even_in(sw, 2, 4096) || !even_in(sh, 2, 4096)) return false;
    for (const h264mi_cell &c : cells) {
        if (c.src < 0 || c.src >= nsrc || c.canvas < 0 || c.canvas >= ncanvas) return false;
        if (!even_in(c.sx, 0, sw) || !even_in(c.sy, 0, sh) || !even_in(c.sw, 2, sw) || !even_in(c.sh, 2, sh)) return false;
        if ((long long)c.sx + c.sw > sw || (long long)c.sy + c.sh > sh) return false;
        if (!even_in(c.dx, 0, cw) || !even_in(c.dy, 0, ch) || !even_in(c.dw, 2, cw) || !even_in(c.dh, 2, ch)) return false;
        if ((long long)c.dx + c.dw > cw || (long long)c.dy + c.dh > ch) return false;
        const bool wider = c.dw > c.sw, taller = c.dh > c.sh, narrower = c.dw < c.sw, shorter = c.dh < c.sh;
        if ((wider && shorter) || (narrower && taller)) return false;
        if ((wider || taller) && !may_enlarge) return false;
    }
    for (size_t i = 0; i < cells.size(); i++)
        for (size_t j = i + 1; j < cells.size(); j++) {
            const h264mi_cell &a = cells[i], &b = cells[j];
            const long long x0 = std::max(a.dx, b.dx), x1 = std::min((long long)a.dx + a.dw, (long long)b.dx + b.dw);
            const long long y0 = std::max(a.dy, b.dy), y1 = std::min((long long)a.dy + a.dh, (long long)b.dy + b.dh);
            if (a.canvas == b.canvas && x0 < x1 && y0 < y1) return false;
        }
    return true;
}

static void verdicts(int cw, int ch, int ncanvas, int sw, int sh, int nsrc, const std::vector<h264mi_cell> &cells, int *refused) {
    const auto p = heap(cells);
    for (int e = 0; e < 2; e++) {
        const bool got = cells_ok(cw, ch, ncanvas, sw, sh, nsrc, p.get(), (int)cells.size(), e != 0);
        CHECK(got == ref_ok(cw, ch, ncanvas, sw, sh, nsrc, cells, e != 0));
        if (!got) refused[e]++;
    }
}

static int *field(h264mi_cell &c, int f) {
    int *p[10] = {&c.src, &c.canvas, &c.sx, &c.sy, &c.sw, &c.sh, &c.dx, &c.dy, &c.dw, &c.dh};
    return p[f];
}

static void check_cells() {
    // the valid lists of tests/test_compose_host.py and tests/test_upscale_host.py, and one with room on every side
    struct Base { int cw, ch, ncanvas, sw, sh, nsrc; std::vector<h264mi_cell> cells; };
    const std::vector<Base> bases = {
        {32, 32, 1, 32, 32, 1, {{0, 0, 0, 0, 32, 32, 0, 0, 16, 16}}},
        {64, 64, 1, 32, 32, 1, {{0, 0, 0, 0, 16, 16, 0, 0, 32, 32}, {0, 0, 0, 0, 32, 32, 32, 32, 16, 16}}},
        {64, 64, 2, 32, 32, 2, {{1, 1, 4, 4, 16, 16, 8, 8, 16, 16}, {0, 0, 2, 2, 8, 8, 4, 4, 16, 16}}},
    };
    int refused[2] = {0, 0}, cases = 0;
    for (const Base &b : bases) {
        verdicts(b.cw, b.ch, b.ncanvas, b.sw, b.sh, b.nsrc, b.cells, refused);
        for (size_t k = 0; k < b.cells.size(); k++)
            for (int f = 0; f < 10; f++) {
                const h264mi_cell &c0 = b.cells[k];
                const int lim[10] = {b.nsrc, b.ncanvas, b.sw, b.sh, b.sw, b.sh, b.cw, b.ch, b.cw, b.ch};
                const int over[10] = {0, 0, b.sw - c0.sw + 2, b.sh - c0.sh + 2, b.sw - c0.sx + 2, b.sh - c0.sy + 2,
                                      b.cw - c0.dw + 2, b.ch - c0.dh + 2, b.cw - c0.dx + 2, b.ch - c0.dy + 2};
                const int values[] = {*field(const_cast<h264mi_cell &>(c0), f) + 1, -2, -1, lim[f], lim[f] + 2, over[f], 2147483646, 0};
                for (int v : values) {
                    Base m = b;
                    *field(m.cells[k], f) = v;
                    verdicts(m.cw, m.ch, m.ncanvas, m.sw, m.sh, m.nsrc, m.cells, refused);
                    cases++;
                }
            }
        // a rectangle larger than its crop on one axis, then on both
        Base m = b;
        m.cells[0] = {0, 0, 0, 0, 8, 8, m.cells[0].dx, m.cells[0].dy, 10, 8};
        verdicts(m.cw, m.ch, m.ncanvas, m.sw, m.sh, m.nsrc, m.cells, refused);
        m.cells[0].dw = 8; m.cells[0].dh = 10;
        verdicts(m.cw, m.ch, m.ncanvas, m.sw, m.sh, m.nsrc, m.cells, refused);
        m.cells[0].dw = 10;
        verdicts(m.cw, m.ch, m.ncanvas, m.sw, m.sh, m.nsrc, m.cells, refused);
        cases += 3;
    }
    // two cells of one canvas touching, sharing one sample (a 2 x 2 corner: fields are even), on different canvases
    const h264mi_cell a{0, 0, 0, 0, 16, 16, 0, 0, 16, 16};
    for (int dx : {16, 14, 0})
        for (int dy : {16, 14, 0})
            for (int canvas : {0, 1}) {
                verdicts(64, 64, 2, 32, 32, 1, {a, {0, canvas, 0, 0, 16, 16, dx, dy, 16, 16}}, refused);
                verdicts(64, 64, 2, 32, 32, 1, {{0, canvas, 0, 0, 16, 16, dx, dy, 16, 16}, a}, refused);
                cases += 2;
            }
    const auto one = heap({a});
    CHECK(!cells_ok(64, 64, 1, 32, 32, 1, nullptr, 1, true) && !cells_ok(64, 64, 1, 32, 32, 1, one.get(), 0, true));
    CHECK(!cells_ok(64, 64, 1, 32, 32, 1, one.get(), -1, true) && !cells_ok(64, 64, 1, 32, 32, 1, one.get(), 4097, false));
    CHECK(!cells_ok(64, 64, 0, 32, 32, 1, one.get(), 1, true) && !cells_ok(64, 64, 1, 32, 32, -1, one.get(), 1, true));
    for (int bad : {0, -2, 31, 8194})
        CHECK(!cells_ok(bad, 64, 1, 32, 32, 1, one.get(), 1, true) && !cells_ok(64, bad, 1, 32, 32, 1, one.get(), 1, true));
    for (int bad : {0, -2, 31, 4098})
        CHECK(!cells_ok(64, 64, 1, bad, 32, 1, one.get(), 1, true) && !cells_ok(64, 64, 1, 32, bad, 1, one.get(), 1, true));
    CHECK(refused[0] > refused[1] && refused[1] > 0);  // the two rules differ, and both refuse
    printf("cells_ok: %d lists, refused %d without enlarging, %d with\n", cases, refused[0], refused[1]);
}

static int waves_a(int dw, int dh) { return ((dw + 63) / 64) * ((dh + 15) / 16) + 2 * ((dw / 2 + 63) / 64) * ((dh / 2 + 15) / 16); }

// n disjoint cells on one 256 x 512 canvas: 4 x 4 rectangles from 2 x 2 crops (enlarging) or 4 x 4 crops (not)
static std::vector<h264mi_cell> grid(int n, bool enlarge) {
    std::vector<h264mi_cell> v;
    for (int k = 0; k < n; k++) v.push_back({k % 3, 0, 2 * (k % 5), 2 * (k % 7), enlarge ? 2 : 4, enlarge ? 2 : 4, 4 * (k % 64), 4 * (k / 64), 4, 4});
    return v;
}

static void check_tables() {
    for (int n : {1, 64, 65, 4096}) {
        const std::vector<h264mi_cell> v = grid(n, false);
        const auto cells = heap(v);
        CHECK(cells_ok(256, 512, 1, 32, 32, 3, cells.get(), n, false) && ref_ok(256, 512, 1, 32, 32, 3, v, false));
        int launches = 0, seen = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {  // the split of launch_compose_i420 and launch_upscale_cells
            const int m = std::min(n - k0, 64);
            std::unique_ptr<PictureCell[]> cell(new PictureCell[m]);
            std::unique_ptr<int[]> first(new int[m + 1]);
            CHECK(fill_cell_table(cell.get(), first.get(), cells.get() + k0, m, waves_a) == m);
            int sum = 0;
            for (int k = 0; k < m; k++) {
                const h264mi_cell &c = v[k0 + k];
                CHECK(first[k] == sum);
                sum += waves_a(c.dw, c.dh);
                CHECK(cell[k].src == c.src && cell[k].canvas == c.canvas && cell[k].sx == c.sx && cell[k].sy == c.sy && cell[k].sw == c.sw &&
                      cell[k].sh == c.sh && cell[k].dx == c.dx && cell[k].dy == c.dy && cell[k].dw == c.dw && cell[k].dh == c.dh);
            }
            CHECK(first[m] == sum && launch_blocks(sum) == (unsigned)std::min((sum + 3) / 4, 2048));
            launches++;
            seen += m;
        }
        CHECK(launches == (n + 63) / 64 && seen == n);
        // a list of both kinds, as launch_compose_any_i420 splits it
        std::vector<h264mi_cell> mixed = grid(n, false), up = grid(n, true);
        int kinds[2] = {0, 0};
        for (int k = 0; k < n; k += 2) mixed[k] = up[k];
        const auto mp = heap(mixed);
        CHECK(cells_ok(256, 512, 1, 32, 32, 3, mp.get(), n, true) && cells_ok(256, 512, 1, 32, 32, 3, mp.get(), n, false) == false);
        for (int k = 0; k < n; k++) kinds[cell_kind(mp[k])]++;
        CHECK(kinds[1] == (n + 1) / 2 && kinds[0] == n / 2);
        // placements: disjoint ones end a launch every 64, a stack of the same rectangle after every one
        std::unique_ptr<h264mi_overlay[]> ov(new h264mi_overlay[n]);
        for (int k = 0; k < n; k++) ov[k] = h264mi_overlay{0, 0, 0, 0, 4, 4, 4 * (k % 64), 4 * (k / 64), 256, 0};
        CHECK(overlay_args_ok(256, 512, 1, 8, 8, 1, ov.get(), n));
        int ends = 0;
        for (int k0 = 0; k0 < n; ends++) {
            const int k1 = overlay_launch_end(ov.get(), n, k0);
            CHECK(k1 == std::min(k0 + 64, n));
            k0 = k1;
        }
        CHECK(ends == (n + 63) / 64);
        for (int k = 0; k < n; k++) { ov[k].dx = 8; ov[k].dy = 8; ov[k].canvas = k & 1; }  // two canvases: pairs are disjoint
        for (int k0 = 0; k0 < n;) {
            const int k1 = overlay_launch_end(ov.get(), n, k0);
            CHECK(k1 == std::min(k0 + 2, n));
            k0 = k1;
        }
    }
    printf("tables and launch splits: lists of 1, 64, 65, 4096\n");
}

static void check_layouts() {
    const int sizes[][4] = {{1920, 1080, 1920, 1080}, {64, 36, 48, 48}, {176, 144, 352, 288}, {4096, 2160, 640, 360}, {32, 32, 32, 32},
                            {1280, 720, 854, 480}, {16, 16, 160, 112}, {36, 18, 50, 22}, {2, 2, 8192, 8192}, {4096, 4096, 8192, 8192}};
    int made = 0, refused = 0;
    for (const auto &s : sizes)
        for (int n : {1, 2, 3, 9, 17, 64, 65, 4096}) {
            std::unique_ptr<h264mi_cell[]> out(new h264mi_cell[n]);
            const int r = mosaic_cells(out.get(), n, n, s[0], s[1], s[2], s[3]);
            CHECK(r == n || r == -1);
            if (r == n) CHECK(cells_ok(s[2], s[3], 1, s[0], s[1], n, out.get(), n, false));
            r == n ? made++ : refused++;
            for (int speaker : {0, n / 2, n - 1}) {
                const int q = speaker_cells(out.get(), n, n, speaker, s[0], s[1], s[2], s[3]);
                CHECK(q == n || q == -1);
                if (q == n) CHECK(cells_ok(s[2], s[3], 1, s[0], s[1], n, out.get(), n, true));
                q == n ? made++ : refused++;
            }
            CHECK(mosaic_cells(out.get(), n - 1, n, s[0], s[1], s[2], s[3]) == -1 && speaker_cells(out.get(), n - 1, n, 0, s[0], s[1], s[2], s[3]) == -1);
            CHECK(speaker_cells(out.get(), n, n, n, s[0], s[1], s[2], s[3]) == -1 && speaker_cells(out.get(), n, n, -1, s[0], s[1], s[2], s[3]) == -1);
        }
    std::unique_ptr<h264mi_cell[]> out(new h264mi_cell[1]);
    CHECK(mosaic_cells(nullptr, 1, 1, 64, 36, 48, 48) == -1 && mosaic_cells(out.get(), 4097, 4097, 64, 36, 48, 48) == -1);
    CHECK(mosaic_cells(out.get(), 1, 0, 64, 36, 48, 48) == -1 && speaker_cells(nullptr, 1, 1, 0, 64, 36, 48, 48) == -1);
    CHECK(speaker_cells(out.get(), 4097, 4097, 0, 64, 36, 48, 48) == -1 && mosaic_cells(out.get(), 1, 1, 63, 36, 48, 48) == -1);
    CHECK(made > 0 && refused > 0);
    printf("mosaic_cells, speaker_cells: %d layouts made and checked, %d refused\n", made, refused);
}

static void check_scalars() {
    CHECK(i420_bytes(32, 32) == 1536 && i420_bytes(6, 4) == 36 && i420a_bytes(32, 32) == 2560 && i420_bytes(8192, 8192) == 100663296u);
    char *base = (char *)0x10000000;
    for (int off : {0, 1, 1535, -1, -1535}) CHECK(i420_ranges_overlap(base + off, 32, 32, 1, base, 32, 32, 1));
    CHECK(!i420_ranges_overlap(base + 1536, 32, 32, 1, base, 32, 32, 1) && !i420_ranges_overlap(base - 1536, 32, 32, 1, base, 32, 32, 1));
    CHECK(i420_ranges_overlap(base + 3 * 1536 - 1, 32, 32, 1, base, 32, 32, 3) && !i420_ranges_overlap(base + 3 * 1536, 32, 32, 1, base, 32, 32, 3));
    CHECK(byte_ranges_overlap(base, 1, base, 1) && !byte_ranges_overlap(base, 1, base + 1, 1) && !byte_ranges_overlap(base, 0, base, 0));
    CHECK(rects_share(0, 0, 2, 2, 0, 0, 2, 2) && !rects_share(0, 0, 2, 2, 2, 0, 2, 2) && !rects_share(0, 0, 2, 2, 0, 2, 2, 2));
    CHECK(scale_args_ok(2, 2, 4096, 4096, 1) && !scale_args_ok(2, 2, 4098, 4096, 1) && !scale_args_ok(34, 32, 32, 32, 1) && !scale_args_ok(0, 2, 32, 32, 1));
    CHECK(!scale_args_ok(16, 16, 32, 32, 0) && !scale_args_ok(15, 16, 32, 32, 1) && scale_args_ok(32, 32, 32, 32, 2147483647));
    CHECK(upscale_args_ok(8192, 8192, 4096, 4096, 1, 0) && !upscale_args_ok(8194, 8192, 4096, 4096, 1, 0) && !upscale_args_ok(30, 32, 32, 32, 1, 1));
    CHECK(!upscale_args_ok(64, 64, 32, 32, 1, 2) && !upscale_args_ok(64, 64, 32, 32, 0, 1) && !upscale_args_ok(8192, 8192, 4098, 32, 1, 1));
    CHECK(fill_args_ok(8192, 2, 1, 0, 255, 0) && !fill_args_ok(8194, 2, 1, 0, 0, 0) && !fill_args_ok(0, 2, 1, 0, 0, 0) && !fill_args_ok(2, 2, 1, 256, 0, 0));
    CHECK(!fill_args_ok(2, 2, 1, 0, -1, 0) && !fill_args_ok(2, 2, 0, 0, 0, 0) && !fill_args_ok(3, 2, 1, 0, 0, 0));
    CHECK(rgba_to_i420a_args_ok(8192, 2, 1) && !rgba_to_i420a_args_ok(8194, 2, 1) && !rgba_to_i420a_args_ok(2, 2, 0) && !rgba_to_i420a_args_ok(2, 3, 1));
    const h264mi_overlay good{0, 0, 0, 0, 4, 4, 4, 4, 256, 0};
    CHECK(overlay_args_ok(8, 8, 1, 8192, 8192, 1, &good, 1) && !overlay_args_ok(8, 8, 1, 8194, 8, 1, &good, 1) && !overlay_args_ok(8, 8, 1, 8, 8, 1, nullptr, 1));
    CHECK(!overlay_args_ok(8, 8, 1, 8, 8, 1, &good, 0) && !overlay_args_ok(8, 8, 1, 8, 8, 1, &good, 4097) && !overlay_args_ok(6, 8, 1, 8, 8, 1, &good, 1));
    h264mi_overlay bad = good;
    bad.dx = 2147483646;
    CHECK(!overlay_args_ok(8, 8, 1, 8, 8, 1, &bad, 1));
    bad = good; bad.opacity = 257;
    CHECK(!overlay_args_ok(8, 8, 1, 8, 8, 1, &bad, 1));
    CHECK(launch_blocks(0) == 0 && launch_blocks(1) == 1 && launch_blocks(8192) == 2048 && launch_blocks(1LL << 40) == 2048);
    printf("scalar checks, byte counts, ranges\n");
}

// orient.hip's host half: the plane restatement in heap blocks of exactly pw * ph bytes against the header's table in
// 64-bit indices, compose and inverse against planes turned twice, the sizes and the scalar check at their limits
static void check_orient() {
    const int sizes[][2] = {{1, 1}, {3, 2}, {2, 3}, {5, 7}, {64, 1}, {1, 64}, {18, 9}};
    for (const auto &s : sizes) {
        const int pw = s[0], ph = s[1];
        std::unique_ptr<uint8_t[]> S(new uint8_t[pw * ph]), D(new uint8_t[pw * ph]), E(new uint8_t[pw * ph]), F(new uint8_t[pw * ph]);
        for (int k = 0; k < pw * ph; k++) S[k] = (uint8_t)(k * 37 + 11);
        for (int a = 0; a < 8; a++) {
            const bool t = a == 1 || a == 3 || a == 6 || a == 7;
            const long long qw = t ? ph : pw, qh = t ? pw : ph;
            orient_plane_host(a, S.get(), pw, ph, D.get());
            for (long long y = 0; y < qh; y++)
                for (long long x = 0; x < qw; x++) {
                    const long long sy[8] = {y, ph - 1 - x, ph - 1 - y, x, y, ph - 1 - y, x, ph - 1 - x};
                    const long long sx[8] = {x, y, pw - 1 - x, pw - 1 - y, pw - 1 - x, x, y, pw - 1 - y};
                    CHECK(D[y * qw + x] == S[sy[a] * pw + sx[a]]);
                }
            for (int b = 0; b < 8; b++) {  // a, then b, in one turn
                const int c = orient_compose(a, b);
                CHECK(c >= 0 && c < 8);
                if (c < 0) continue;
                orient_plane_host(b, D.get(), (int)qw, (int)qh, E.get());
                orient_plane_host(c, S.get(), pw, ph, F.get());
                CHECK(std::equal(E.get(), E.get() + pw * ph, F.get()));
            }
            orient_plane_host(orient_inverse(a), D.get(), (int)qw, (int)qh, E.get());
            CHECK(std::equal(E.get(), E.get() + pw * ph, S.get()));
        }
    }
    int dw = -7, dh = -7;
    for (int bad : {-1, 8, 2147483647}) {
        CHECK(orient_compose(bad, 0) == -1 && orient_compose(0, bad) == -1 && orient_inverse(bad) == -1);
        CHECK(orient_size(bad, 16, 16, &dw, &dh) == -1 && !orient_args_ok(bad, 16, 16, 1));
    }
    for (int bad : {0, -2, 15, 8194, 2147483647}) {
        CHECK(orient_size(1, bad, 16, &dw, &dh) == -1 && orient_size(1, 16, bad, &dw, &dh) == -1);
        CHECK(!orient_args_ok(1, bad, 16, 1) && !orient_args_ok(0, 16, bad, 1));
    }
    CHECK(orient_size(1, 16, 16, nullptr, &dh) == -1 && orient_size(1, 16, 16, &dw, nullptr) == -1 && dw == -7 && dh == -7);
    CHECK(orient_size(1, 8192, 2, &dw, &dh) == 0 && dw == 2 && dh == 8192 && orient_size(4, 8192, 2, &dw, &dh) == 0 && dw == 8192 && dh == 2);
    CHECK(orient_args_ok(7, 8192, 8192, 2147483647) && !orient_args_ok(7, 16, 16, 0) && !orient_args_ok(7, 16, 16, -1));
    printf("orient: the plane restatement, compose, inverse on 7 sizes, the scalar checks\n");
}

// the layout rules of include/h264mi.h restated in 128-bit arithmetic, one predicate per rule; the span, or -1
static __int128 ref_pix_span(const h264mi_pix_layout &L, long long w, long long h) {
    if (w % 2 || h % 2 || w < 2 || h < 2 || w > 8192 || h > 8192) return -1;
    __int128 rb[3], rows[3], unit = 1;
    int np;
    switch (L.pix) {
    case 0: np = 3; rb[0] = w; rows[0] = h; rb[1] = rb[2] = w / 2; rows[1] = rows[2] = h / 2; break;
    case 1: case 2: np = 2; rb[0] = w; rows[0] = h; rb[1] = w; rows[1] = h / 2; break;
    case 3: case 4: np = 1; rb[0] = 2 * w; rows[0] = h; break;
    // the table of ids 16..24: I422, I444, NV16, Y800, P010, I010, P210, I210, V210
    case 16: np = 3; rb[0] = w; rb[1] = rb[2] = w / 2; rows[0] = rows[1] = rows[2] = h; break;
    case 17: np = 3; rb[0] = rb[1] = rb[2] = w; rows[0] = rows[1] = rows[2] = h; break;
    case 18: np = 2; rb[0] = rb[1] = w; rows[0] = rows[1] = h; break;
    case 19: np = 1; rb[0] = w; rows[0] = h; break;
    case 20: np = 2; unit = 2; rb[0] = rb[1] = 2 * w; rows[0] = h; rows[1] = h / 2; break;
    case 21: np = 3; unit = 2; rb[0] = 2 * w; rb[1] = rb[2] = w; rows[0] = h; rows[1] = rows[2] = h / 2; break;
    case 22: np = 2; unit = 2; rb[0] = rb[1] = 2 * w; rows[0] = rows[1] = h; break;
    case 23: np = 3; unit = 2; rb[0] = 2 * w; rb[1] = rb[2] = w; rows[0] = rows[1] = rows[2] = h; break;
    case 24: np = 1; unit = 4; rb[0] = 16 * ((w + 5) / 6); rows[0] = h; break;
    default: return -1;
    }
    for (int p = 0; p < np; p++)
        if ((__int128)L.pitch[p] % unit != 0 || (__int128)L.offset[p] % unit != 0) return -1;  // the unit rule
    __int128 lo[3], hi[3], span = 0;
    for (int p = 0; p < 3; p++) {
        if (p >= np) {
            if (L.pitch[p] != 0 || L.offset[p] != 0) return -1;
            continue;
        }
        if (L.pitch[p] < rb[p] || L.pitch[p] > 65536 || L.offset[p] < 0) return -1;
        lo[p] = L.offset[p];
        hi[p] = lo[p] + (rows[p] - 1) * L.pitch[p] + rb[p];
        if (hi[p] > span) span = hi[p];
    }
    for (int p = 0; p < np; p++)
        for (int q = p + 1; q < np; q++)
            if (lo[p] < hi[q] && lo[q] < hi[p]) return -1;
    return span > (__int128)INT64_MAX ? (__int128)-1 : span;
}

static uint64_t pix_rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t pix_rng() {  // xorshift64
    pix_rng_state ^= pix_rng_state << 13; pix_rng_state ^= pix_rng_state >> 7; pix_rng_state ^= pix_rng_state << 17;
    return pix_rng_state;
}

static void check_pix() {
    // tight layouts and spans of the five formats: bytes per frame 12 or 16 bits a sample, planes back to back
    const int sizes[][2] = {{2, 2}, {36, 18}, {1280, 720}, {8192, 8192}, {8192, 2}, {2, 8192}};
    for (const auto &s : sizes)
        for (int pix = 0; pix < 5; pix++) {
            std::unique_ptr<h264mi_pix_layout> L(new h264mi_pix_layout);
            const long long w = s[0], h = s[1], bytes = pix >= 3 ? 2 * w * h : w * h + 2 * (w / 2) * (h / 2);
            CHECK(pix_layout_tight(L.get(), pix, s[0], s[1]) == 0);
            CHECK(L->pix == pix && L->frame_stride == bytes && pix_span(L.get(), s[0], s[1]) == bytes && pix_layout_ok(L.get(), s[0], s[1]));
            CHECK(ref_pix_span(*L, w, h) == bytes && L->offset[0] == 0);
            CHECK(L->pitch[0] == (pix >= 3 ? 2 * w : w) && L->offset[1] == (pix >= 3 ? 0 : w * h));
            CHECK(L->pitch[1] == (pix == 0 ? w / 2 : pix >= 3 ? 0 : w) && L->pitch[2] == (pix == 0 ? w / 2 : 0));
            CHECK(L->offset[2] == (pix == 0 ? w * h + (w / 2) * (h / 2) : 0));
            CHECK(pix == 0 ? (size_t)bytes == i420_bytes(s[0], s[1]) : true);
            h264mi_pix_layout m = *L;
            m.frame_stride--;
            CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == bytes);
            m = *L; m.pitch[0]--;
            CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == -1);
        }
    h264mi_pix_layout keep{7, {7, 7, 7}, {7, 7, 7}, 7};
    for (int bad : {-1, 5, 2147483647}) CHECK(pix_layout_tight(&keep, bad, 16, 16) == -1);
    for (int bad : {0, -2, 15, 8194, 2147483647}) CHECK(pix_layout_tight(&keep, 0, bad, 16) == -1 && pix_layout_tight(&keep, 3, 16, bad) == -1);
    CHECK(pix_layout_tight(nullptr, 0, 16, 16) == -1 && keep.pix == 7 && keep.pitch[2] == 7 && keep.offset[0] == 7 && keep.frame_stride == 7);
    CHECK(pix_span(nullptr, 16, 16) == -1 && !pix_layout_ok(nullptr, 16, 16) && !pix_args_ok(nullptr, 16, 16, 1));
    // random and extreme fields against the restatement
    const int32_t e32[] = {0, 1, -1, 2147483647, -2147483647 - 1, 65536, 65537, 16, 18, 36, 72};
    const int64_t e64[] = {0, 1, -1, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MAX - 647, 1LL << 31, 1LL << 32, 648, 810, 972, 1296};
    int good = 0, cases = 0;
    for (int it = 0; it < 200000; it++) {
        std::unique_ptr<h264mi_pix_layout> L(new h264mi_pix_layout);  // a heap block of exactly the struct
        int w = 36, h = 18;
        if (it % 2) {  // every field random, the extremes mixed in
            L->pix = (int)(pix_rng() % 7) - 1;
            for (int p = 0; p < 3; p++) {
                L->pitch[p] = pix_rng() % 3 ? (int32_t)(pix_rng() % 200) : e32[pix_rng() % (sizeof e32 / sizeof *e32)];
                L->offset[p] = pix_rng() % 3 ? (int64_t)(pix_rng() % 3000) : e64[pix_rng() % (sizeof e64 / sizeof *e64)];
            }
            L->frame_stride = pix_rng() % 3 ? (int64_t)(pix_rng() % 6000) : e64[pix_rng() % (sizeof e64 / sizeof *e64)];
            if (pix_rng() % 8 == 0) w = e32[pix_rng() % (sizeof e32 / sizeof *e32)];
            if (pix_rng() % 8 == 0) h = e32[pix_rng() % (sizeof e32 / sizeof *e32)];
        } else {  // a tight layout with one field moved a little or to an extreme
            CHECK(pix_layout_tight(L.get(), (int)(pix_rng() % 5), w, h) == 0);
            const int f = (int)(pix_rng() % 8);
            const bool ext = pix_rng() % 4 == 0;
            const int d = (int)(pix_rng() % 81) - 40;
            if (f < 3) L->pitch[f] = ext ? e32[pix_rng() % (sizeof e32 / sizeof *e32)] : L->pitch[f] + d;
            else if (f < 6) L->offset[f - 3] = ext ? e64[pix_rng() % (sizeof e64 / sizeof *e64)] : L->offset[f - 3] + d;
            else if (f == 6) L->frame_stride = ext ? e64[pix_rng() % (sizeof e64 / sizeof *e64)] : L->frame_stride + d;
        }
        const __int128 want = ref_pix_span(*L, w, h);
        const int64_t got = pix_span(L.get(), w, h);
        CHECK((__int128)got == want);
        const bool ok = want >= 0 && (__int128)L->frame_stride >= want;
        CHECK(pix_layout_ok(L.get(), w, h) == ok);
        CHECK(pix_args_ok(L.get(), w, h, 1) == ok && !pix_args_ok(L.get(), w, h, 0) && !pix_args_ok(L.get(), w, h, -1));
        if (ok) {  // the range test of a call: n frames of the layout against n tight frames, in 128 bits
            const int n = 1 + (int)(pix_rng() % 3);
            const uintptr_t a0 = 0x10000000u, b0 = pix_rng() % 2 ? a0 + (uintptr_t)(pix_rng() % 8000) : a0 - (uintptr_t)(pix_rng() % 8000);
            const unsigned __int128 ab = (unsigned __int128)L->frame_stride * n, bb = (unsigned __int128)i420_bytes(w, h) * n;
            const bool share = (ab >> 63) != 0 || ((unsigned __int128)a0 < b0 + bb && (unsigned __int128)b0 < a0 + ab);
            CHECK(pix_ranges_overlap((const void *)a0, *L, (const void *)b0, w, h, n) == share);
        }
        good += ok;
        cases++;
    }
    CHECK(good > cases / 20 && good < cases - cases / 20);
    printf("pixel layouts: tight layouts of 5 formats x 6 sizes, %d random and extreme layouts (%d good)\n", cases, good);
}

static int ref_pix_unit(int pix) { return (pix >= 0 && pix <= 4) || (pix >= 16 && pix <= 19) ? 1 : pix >= 20 && pix <= 23 ? 2 : pix == 24 ? 4 : -1; }

// the formats 16..24 and the unit rule: tight layouts, then random and extreme fields against the restatement
static void check_pixdeep() {
    const int sizes[][2] = {{2, 2}, {6, 2}, {36, 18}, {50, 2}, {1280, 720}, {8192, 8192}, {8192, 2}, {2, 8192}};
    const int bits[9] = {16, 24, 16, 8, 24, 24, 32, 32, 0};
    for (const auto &s : sizes)
        for (int pix = 16; pix <= 24; pix++) {
            std::unique_ptr<h264mi_pix_layout> L(new h264mi_pix_layout);
            const long long w = s[0], h = s[1];
            CHECK(pix_layout_tight(L.get(), pix, s[0], s[1]) == 0 && L->pix == pix && L->offset[0] == 0 && pix_layout_ok(L.get(), s[0], s[1]));
            const long long span = pix == 24 ? (h - 1) * 128 * ((w + 47) / 48) + 16 * ((w + 5) / 6) : w * h * bits[pix - 16] / 8;
            CHECK(pix_span(L.get(), s[0], s[1]) == span && ref_pix_span(*L, w, h) == span);
            CHECK(L->frame_stride == (pix == 24 ? h * 128 * ((w + 47) / 48) : span) && L->frame_stride % ref_pix_unit(pix) == 0);
            if (pix == 24) CHECK(L->pitch[0] == 128 * ((w + 47) / 48) && L->pitch[0] <= 65536);
            h264mi_pix_layout m = *L;
            m.frame_stride = span - ref_pix_unit(pix);
            CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == span);
            for (int d = 1; d < ref_pix_unit(pix); d++) {  // the unit rule, field by field
                m = *L; m.frame_stride += d;
                CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == span);
                m = *L; m.offset[0] += d; m.frame_stride = INT64_MAX - 3;
                CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == -1);
                m = *L; m.pitch[0] += d; m.frame_stride = INT64_MAX - 3;
                CHECK(!pix_layout_ok(&m, s[0], s[1]) && pix_span(&m, s[0], s[1]) == -1);
                CHECK(!pix_base_ok((const void *)(uintptr_t)(0x10000000u + d), *L));
            }
            CHECK(pix_base_ok((const void *)(uintptr_t)0x10000000u, *L) && pix_base_ok((const void *)(uintptr_t)(0x10000000u + 4), *L));
        }
    for (int pix = -2; pix <= 30; pix++) CHECK(pix_unit(pix) == ref_pix_unit(pix) && (pix_planes(pix) == 0) == (ref_pix_unit(pix) < 0));
    CHECK(pix_unit(INT32_MAX) == -1 && pix_unit(INT32_MIN) == -1);
    h264mi_pix_layout keep{7, {7, 7, 7}, {7, 7, 7}, 7};
    for (int bad = 5; bad <= 15; bad++) CHECK(pix_layout_tight(&keep, bad, 16, 16) == -1);
    CHECK(pix_layout_tight(&keep, 25, 16, 16) == -1 && keep.pix == 7 && keep.frame_stride == 7);
    const int32_t e32[] = {0, 1, -1, 2, 2147483647, -2147483647 - 1, 65536, 65537, 65534, 16, 18, 36, 72, 96, 144};
    const int64_t e64[] = {0, 1, -1, 2, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MAX - 3, INT64_MAX - 647, 1LL << 31, 1LL << 32, 648, 1296, 2592};
    int good = 0, cases = 0;
    for (int it = 0; it < 200000; it++) {
        std::unique_ptr<h264mi_pix_layout> L(new h264mi_pix_layout);  // a heap block of exactly the struct
        int w = 36, h = 18;
        if (it % 2) {
            L->pix = 14 + (int)(pix_rng() % 13);
            for (int p = 0; p < 3; p++) {
                L->pitch[p] = pix_rng() % 3 ? (int32_t)(pix_rng() % 300) : e32[pix_rng() % (sizeof e32 / sizeof *e32)];
                L->offset[p] = pix_rng() % 3 ? (int64_t)(pix_rng() % 6000) : e64[pix_rng() % (sizeof e64 / sizeof *e64)];
            }
            L->frame_stride = pix_rng() % 3 ? (int64_t)(pix_rng() % 12000) : e64[pix_rng() % (sizeof e64 / sizeof *e64)];
            if (pix_rng() % 8 == 0) w = e32[pix_rng() % (sizeof e32 / sizeof *e32)];
            if (pix_rng() % 8 == 0) h = e32[pix_rng() % (sizeof e32 / sizeof *e32)];
        } else {  // a tight layout with one field moved a little or to an extreme
            CHECK(pix_layout_tight(L.get(), 16 + (int)(pix_rng() % 9), w, h) == 0);
            const int f = (int)(pix_rng() % 9);
            const bool ext = pix_rng() % 4 == 0;
            const int d = (int)(pix_rng() % 17) - 8;
            if (f < 3) L->pitch[f] = ext ? e32[pix_rng() % (sizeof e32 / sizeof *e32)] : L->pitch[f] + d;
            else if (f < 6) L->offset[f - 3] = ext ? e64[pix_rng() % (sizeof e64 / sizeof *e64)] : L->offset[f - 3] + d;
            else if (f == 6) L->frame_stride = ext ? e64[pix_rng() % (sizeof e64 / sizeof *e64)] : L->frame_stride + d;
        }
        const __int128 want = ref_pix_span(*L, w, h);
        CHECK((__int128)pix_span(L.get(), w, h) == want);
        const bool ok = want >= 0 && (__int128)L->frame_stride >= want && (__int128)L->frame_stride % ref_pix_unit(L->pix) == 0;
        CHECK(pix_layout_ok(L.get(), w, h) == ok);
        CHECK(pix_args_ok(L.get(), w, h, 1) == ok && !pix_args_ok(L.get(), w, h, 0));
        if (ok) {
            const int n = 1 + (int)(pix_rng() % 3);
            const uintptr_t a0 = 0x10000000u, b0 = pix_rng() % 2 ? a0 + (uintptr_t)(pix_rng() % 16000) : a0 - (uintptr_t)(pix_rng() % 16000);
            const unsigned __int128 ab = (unsigned __int128)L->frame_stride * n, bb = (unsigned __int128)i420_bytes(w, h) * n;
            const bool share = (ab >> 63) != 0 || ((unsigned __int128)a0 < b0 + bb && (unsigned __int128)b0 < a0 + ab);
            CHECK(pix_ranges_overlap((const void *)a0, *L, (const void *)b0, w, h, n) == share);
        }
        good += ok;
        cases++;
    }
    CHECK(good > cases / 20 && good < cases - cases / 20);
    // h264mi_pixopt: depth 0..2, reserved all zero
    for (int depth = -2; depth <= 4; depth++) {
        std::unique_ptr<h264mi_pixopt> o(new h264mi_pixopt{depth, {0, 0, 0}});
        CHECK(pixopt_ok(o.get()) == (depth >= 0 && depth <= 2));
        for (int k = 0; k < 3; k++)
            for (int32_t v : {1, -1, INT32_MAX, INT32_MIN}) {
                h264mi_pixopt q = *o;
                q.reserved[k] = v;
                CHECK(!pixopt_ok(&q));
            }
    }
    const h264mi_pixopt lo{INT32_MIN, {0, 0, 0}}, hi{INT32_MAX, {0, 0, 0}};
    CHECK(!pixopt_ok(nullptr) && !pixopt_ok(&lo) && !pixopt_ok(&hi));
    printf("deep pixel layouts: tight layouts of 9 formats x 8 sizes with the unit rule, %d random and extreme layouts (%d good), pixopt\n", cases, good);
}

// the sample rule and the gate restated sample by sample: every sample looks its own block up
static void ref_denoise(std::vector<uint8_t> &out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_denoise &p, uint32_t *st) {
    const int nbx = (w + 7) / 8, nby = (h + 7) / 8;
    std::vector<long long> sad((size_t)nbx * nby, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) sad[(size_t)(y / 8) * nbx + x / 8] += llabs((long long)cur[(size_t)y * w + x] - prev[(size_t)y * w + x]);
    st[0] = st[2] = st[3] = 0;
    st[1] = (uint32_t)(nbx * nby);
    auto moving = [&](int bx, int by) {
        const long long bw = std::min(8, w - 8 * bx), bh = std::min(8, h - 8 * by);
        return 4 * sad[(size_t)by * nbx + bx] > (long long)p.motion * bw * bh;
    };
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) st[0] += moving(bx, by);
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    for (size_t i = 0; i < ly + 2 * lc; i++) {
        const int pl = i < ly ? 0 : i < ly + lc ? 1 : 2;
        const size_t j = i - (pl == 0 ? 0 : pl == 1 ? ly : ly + lc);
        const int pw = pl ? w / 2 : w, x = (int)(j % pw), y = (int)(j / pw);
        const bool mv = pl ? moving(x / 4, y / 4) : moving(x / 8, y / 8);
        const int K = pl ? p.strength_c : p.strength_y, c = cur[i], d = c - prev[i], a = d < 0 ? -d : d;
        int m = 0;
        if (!mv && a < p.reach) m = (a * ((K * (p.reach - a)) / p.reach) + 128) >> 8;
        st[pl ? 3 : 2] += (uint32_t)m;
        out[i] = (uint8_t)(d < 0 ? c + m : c - m);
    }
}

static void check_denoise() {
    const int sizes[][2] = {{2, 2}, {8, 8}, {10, 6}, {16, 16}, {36, 18}, {130, 66}, {264, 10}};
    const h264mi_denoise sets[] = {{224, 224, 32, 1020}, {128, 64, 12, 24}, {224, 0, 12, 24}, {0, 0, 12, 24}, {128, 128, 1, 24}, {128, 128, 12, 0}};
    int frames = 0;
    for (const auto &s : sizes)
        for (const h264mi_denoise &p : sets) {
            const int w = s[0], h = s[1];
            const size_t fb = i420_bytes(w, h);
            std::unique_ptr<uint8_t[]> cur(new uint8_t[fb]), prev(new uint8_t[fb]), out(new uint8_t[fb]);  // exactly the frame's bytes
            for (size_t i = 0; i < fb; i++) {
                prev[i] = (uint8_t)pix_rng();
                const int blk = (int)(i / 8) % 4;  // runs of 8 bytes: every fourth far from prev
                cur[i] = blk == 3 ? (uint8_t)pix_rng() : (uint8_t)std::min(255, std::max(0, (int)prev[i] + (int)(pix_rng() % 11) - 5));
            }
            std::vector<uint8_t> want(fb);
            uint32_t st_want[4], st[4] = {9, 9, 9, 9};
            ref_denoise(want, cur.get(), prev.get(), w, h, p, st_want);
            denoise_frame_host(out.get(), cur.get(), prev.get(), w, h, p, st);
            CHECK(memcmp(out.get(), want.data(), fb) == 0);
            CHECK(memcmp(st, st_want, sizeof st) == 0);
            for (size_t i = 0; i < fb; i++) CHECK(std::min(cur[i], prev[i]) <= out[i] && out[i] <= std::max(cur[i], prev[i]));
            denoise_frame_host(prev.get(), cur.get(), prev.get(), w, h, p, nullptr);  // in place over prev
            CHECK(memcmp(prev.get(), want.data(), fb) == 0);
            frames++;
        }
    // the tables: k at the limits, 0 from the reach on, m <= a for every entry
    for (int K : {0, 1, 128, 224})
        for (int T : {1, 2, 12, 31, 32}) {
            std::unique_ptr<DenoiseTables> t(new DenoiseTables);
            const h264mi_denoise p{K, 224 - K, T, 0};
            denoise_tables(t.get(), p);
            for (int a = 0; a < 32; a++) {
                const int ky = (t->k[a / 4] >> (8 * (a % 4))) & 255, kc = (t->k[8 + a / 4] >> (8 * (a % 4))) & 255;
                CHECK(ky == (a < T ? K * (T - a) / T : 0) && kc == (a < T ? (224 - K) * (T - a) / T : 0));
                CHECK(ky <= 224 && kc <= 224 && ((a * ky + 128) >> 8) <= a && ((a * kc + 128) >> 8) <= a);
            }
            CHECK((t->k[0] & 255) == (uint32_t)K);
        }
    // the scalar checks at their limits and one past each
    const h264mi_denoise lo{0, 0, 1, 0}, hi{224, 224, 32, 1020};
    CHECK(denoise_ok(&lo) && denoise_ok(&hi) && !denoise_ok(nullptr));
    for (int f = 0; f < 4; f++) {
        h264mi_denoise a = lo, b = hi;
        ((int32_t *)&a)[f]--; ((int32_t *)&b)[f]++;
        CHECK(!denoise_ok(&a) && !denoise_ok(&b));
        a = lo; ((int32_t *)&a)[f] = INT32_MIN; b = hi; ((int32_t *)&b)[f] = INT32_MAX;
        CHECK(!denoise_ok(&a) && !denoise_ok(&b));
    }
    const uintptr_t D = 0x10000000u, D2 = 0x20000000u, C = 0x30000000u, P = 0x40000000u, S = 0x50000000u;
    auto ok = [&](uintptr_t d, uintptr_t d2, uintptr_t c, uintptr_t p, int w, int h, int n, const h264mi_denoise *q, uintptr_t s) {
        return denoise_args_ok((const void *)d, (const void *)d2, (const void *)c, (const void *)p, w, h, n, q, (const void *)s);
    };
    const size_t nb = 3 * i420_bytes(32, 16);
    CHECK(ok(D, D2, C, P, 32, 16, 3, &hi, S) && ok(D, 0, C, P, 32, 16, 3, &hi, 0) && ok(D, D2, C, P, 8192, 8192, 1, &lo, S) && ok(D, 0, C, P, 2, 2, 1, &lo, 0));
    CHECK(ok(C, 0, C, P, 32, 16, 3, &hi, S) && ok(P, 0, C, P, 32, 16, 3, &hi, S) && ok(C, P, C, P, 32, 16, 3, &hi, S) && ok(P, C, C, P, 32, 16, 3, &hi, S));
    CHECK(ok(D, 0, C, C, 32, 16, 3, &hi, S) && ok(C, 0, C, C, 32, 16, 3, &hi, S));
    CHECK(!ok(0, D2, C, P, 32, 16, 3, &hi, S) && !ok(D, D2, 0, P, 32, 16, 3, &hi, S) && !ok(D, D2, C, 0, 32, 16, 3, &hi, S) && !ok(D, D2, C, P, 32, 16, 3, nullptr, S));
    CHECK(!ok(D, D2, C, P, 32, 16, 0, &hi, S) && !ok(D, D2, C, P, 31, 16, 3, &hi, S) && !ok(D, D2, C, P, 32, 8194, 3, &hi, S) && !ok(D, D2, C, P, 0, 16, 3, &hi, S));
    CHECK(!ok(D, D, C, P, 32, 16, 3, &hi, S) && !ok(C, C, C, P, 32, 16, 3, &hi, S));
    for (uintptr_t off : {(uintptr_t)1, (uintptr_t)(nb - 1), (uintptr_t)-1, (uintptr_t)-(intptr_t)(nb - 1)}) {
        CHECK(!ok(C + off, D2, C, P, 32, 16, 3, &hi, S) && !ok(P + off, D2, C, P, 32, 16, 3, &hi, S) && !ok(D2 + off, D2, C, P, 32, 16, 3, &hi, S));
        CHECK(!ok(D, C + off, C, P, 32, 16, 3, &hi, S) && !ok(D, P + off, C, P, 32, 16, 3, &hi, S) && !ok(D, D2, P + off, P, 32, 16, 3, &hi, S));
    }
    CHECK(ok(D, D2, C, P, 32, 16, 3, &hi, D + nb) && ok(D, D2, C, P, 32, 16, 3, &hi, D - 48));  // touching
    for (uintptr_t b : {D, D2, C, P}) CHECK(!ok(D, D2, C, P, 32, 16, 3, &hi, b) && !ok(D, D2, C, P, 32, 16, 3, &hi, b + nb - 4) && !ok(D, D2, C, P, 32, 16, 3, &hi, b - 44));
    for (uintptr_t off : {1, 2, 3}) CHECK(!ok(D, D2, C, P, 32, 16, 3, &hi, S + off));
    printf("denoise: %d frames at 7 sizes x 6 parameter sets out of place and in place, tables, scalar and range checks\n", frames);
}

// the rule restated sample by sample in another shape: every output sample looks its own plane, line and taps up
static int ref_deint_sample(const uint8_t *C, const uint8_t *P, int pw, int ph, int x, int y, const h264mi_deinterlace &p) {
    const long long v = C[(size_t)y * pw + x];
    if (y % 2 == p.parity) return (int)v;
    const bool hu = y - 1 >= 0, hd = y + 1 < ph;
    if (!hu && !hd) return (int)v;
    auto at = [&](int yy, long long xx) { return (long long)C[(size_t)yy * pw + (size_t)std::min<long long>(std::max<long long>(xx, 0), pw - 1)]; };
    long long s;
    if (hu != hd) {
        s = at(hu ? y - 1 : y + 1, x);
    } else {
        long long score[3];  // d = -1, 0, +1
        for (int d = -1; d <= 1; d++) score[d + 1] = llabs(at(y - 1, x - 1 + d) - at(y + 1, x - 1 - d)) + llabs(at(y - 1, x + d) - at(y + 1, x - d)) +
                                                     llabs(at(y - 1, x + 1 + d) - at(y + 1, x + 1 - d));
        int d = 0;
        if (p.spatial) {
            if (score[0] < score[1]) d = -1;
            if (score[2] < score[1] && score[2] < score[0]) d = 1;
        }
        s = (at(y - 1, x + d) + at(y + 1, x - d) + 1) / 2;
    }
    if (p.temporal && P) {
        const int k = (y ^ 1) < ph ? (y ^ 1) : y;
        const long long m = std::max(llabs(v - P[(size_t)y * pw + x]), llabs((long long)C[(size_t)k * pw + x] - P[(size_t)k * pw + x]));
        s = std::min(std::max(s, v - m), v + m);
    }
    return (int)s;
}
static void ref_deinterlace(std::vector<uint8_t> &out, const uint8_t *cur, const uint8_t *prev, int w, int h, const h264mi_deinterlace &p, uint32_t *st) {
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    st[0] = st[1] = st[2] = st[3] = 0;
    for (size_t i = 0; i < ly + 2 * lc; i++) {
        const int pl = i < ly ? 0 : i < ly + lc ? 1 : 2;
        const size_t base = pl == 0 ? 0 : pl == 1 ? ly : ly + lc, j = i - base;
        const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h, x = (int)(j % pw), y = (int)(j / pw);
        const int o = ref_deint_sample(cur + base, prev ? prev + base : nullptr, pw, ph, x, y, p), v = cur[i];
        CHECK(o >= 0 && o <= 255);
        out[i] = (uint8_t)o;
        const bool missing = y % 2 != p.parity && ph > 1;
        if (!missing) { CHECK(o == v); continue; }
        st[pl ? 3 : 2] += (uint32_t)abs(o - v);
        if (pl == 0) {
            st[0]++;
            if (y >= 1 && y + 1 < ph) {
                const int du = v - cur[i - pw], dd = v - cur[i + pw];
                if ((long long)du * dd > 0 && std::min(abs(du), abs(dd)) > p.comb_level) st[1]++;
            }
        }
    }
}

static void check_deinterlace() {
    const int sizes[][2] = {{2, 2}, {4, 2}, {16, 16}, {18, 10}, {34, 6}, {258, 18}, {528, 34}, {2, 18}};
    int frames = 0;
    for (const auto &s : sizes)
        for (int par = 0; par < 8; par++)
            for (int with_prev = 0; with_prev < 2; with_prev++) {
                const h264mi_deinterlace p{par & 1, (par >> 1) & 1, (par >> 2) & 1, 8};
                const int w = s[0], h = s[1];
                const size_t fb = i420_bytes(w, h);
                std::unique_ptr<uint8_t[]> cur(new uint8_t[fb]), prev(new uint8_t[fb]), out(new uint8_t[fb]);  // exactly the frame's bytes
                for (size_t i = 0; i < fb; i++) {
                    prev[i] = (i / 5) % 3 ? (uint8_t)pix_rng() : (uint8_t)(i % 256);  // runs of a ramp: ties
                    const int kind = (int)(i / 8) % 3;  // runs of 8 bytes: fresh, equal, near
                    cur[i] = kind == 0 ? (uint8_t)pix_rng() : kind == 1 ? prev[i] : (uint8_t)std::min(255, std::max(0, (int)prev[i] + (int)(pix_rng() % 13) - 6));
                }
                const uint8_t *pv = with_prev ? prev.get() : nullptr;
                std::vector<uint8_t> want(fb);
                uint32_t st_want[4], st[4] = {9, 9, 9, 9};
                ref_deinterlace(want, cur.get(), pv, w, h, p, st_want);
                deinterlace_frame_host(out.get(), cur.get(), pv, w, h, p, st);
                CHECK(memcmp(out.get(), want.data(), fb) == 0);
                CHECK(memcmp(st, st_want, sizeof st) == 0 && st[0] == (uint32_t)(w * (h / 2)));
                deinterlace_frame_host(cur.get(), cur.get(), pv, w, h, p, nullptr);  // in place
                CHECK(memcmp(cur.get(), want.data(), fb) == 0);
                frames++;
            }
    // the scalar checks at their limits and one past each
    const h264mi_deinterlace lo{0, 0, 0, 0}, hi{1, 1, 1, 255};
    CHECK(deinterlace_ok(&lo) && deinterlace_ok(&hi) && !deinterlace_ok(nullptr));
    for (int f = 0; f < 4; f++) {
        h264mi_deinterlace a = lo, b = hi;
        ((int32_t *)&a)[f]--; ((int32_t *)&b)[f]++;
        CHECK(!deinterlace_ok(&a) && !deinterlace_ok(&b));
        a = lo; ((int32_t *)&a)[f] = INT32_MIN; b = hi; ((int32_t *)&b)[f] = INT32_MAX;
        CHECK(!deinterlace_ok(&a) && !deinterlace_ok(&b));
    }
    const uintptr_t D = 0x10000000u, Q = 0x20000000u, C = 0x30000000u, P = 0x40000000u, S = 0x50000000u;
    auto ok = [&](uintptr_t d, uintptr_t q, uintptr_t c, uintptr_t p, int w, int h, int n, const h264mi_deinterlace *par, uintptr_t s) {
        return deinterlace_args_ok((const void *)d, (const void *)q, (const void *)c, (const void *)p, w, h, n, par, (const void *)s);
    };
    const size_t nb = 3 * i420_bytes(32, 16), fb = i420_bytes(32, 16);
    CHECK(ok(D, Q, C, P, 32, 16, 3, &hi, S) && ok(D, 0, C, 0, 32, 16, 3, &hi, 0) && ok(D, Q, C, P, 8192, 8192, 1, &lo, S) && ok(D, 0, C, 0, 2, 2, 1, &lo, 0));
    CHECK(ok(C, 0, C, P, 32, 16, 3, &hi, S) && ok(D, P, C, P, 32, 16, 3, &hi, S) && ok(C, P, C, P, 32, 16, 3, &hi, S) && ok(D, Q, C, 0, 32, 16, 3, &hi, S));
    CHECK(ok(D, Q, C, C - fb, 32, 16, 3, &hi, S) && ok(D, Q, C, C, 32, 16, 3, &hi, S) && ok(D, 0, C, C + 1, 32, 16, 3, &hi, 0));  // the read ranges overlap
    CHECK(!ok(C, Q, C, C - fb, 32, 16, 3, &hi, S) && !ok(D, C - fb, C, C - fb, 32, 16, 3, &hi, S) && !ok(C, 0, C, C, 32, 16, 3, &hi, 0));  // one written
    CHECK(!ok(0, Q, C, P, 32, 16, 3, &hi, S) && !ok(D, Q, 0, P, 32, 16, 3, &hi, S) && !ok(D, Q, C, P, 32, 16, 3, nullptr, S));
    CHECK(!ok(D, Q, C, P, 32, 16, 0, &hi, S) && !ok(D, Q, C, P, 31, 16, 3, &hi, S) && !ok(D, Q, C, P, 32, 8194, 3, &hi, S) && !ok(D, Q, C, P, 0, 16, 3, &hi, S));
    CHECK(!ok(D, D, C, P, 32, 16, 3, &hi, S) && !ok(P, Q, C, P, 32, 16, 3, &hi, S) && !ok(D, C, C, P, 32, 16, 3, &hi, S));
    for (uintptr_t off : {(uintptr_t)1, (uintptr_t)(nb - 1), (uintptr_t)-1, (uintptr_t)-(intptr_t)(nb - 1)}) {
        CHECK(!ok(C + off, Q, C, P, 32, 16, 3, &hi, S) && !ok(P + off, Q, C, P, 32, 16, 3, &hi, S) && !ok(Q + off, Q, C, P, 32, 16, 3, &hi, S));
        CHECK(!ok(D, C + off, C, P, 32, 16, 3, &hi, S) && !ok(D, P + off, C, P, 32, 16, 3, &hi, S) && !ok(D, D + off, C, P, 32, 16, 3, &hi, S));
    }
    CHECK(ok(D, Q, C, P, 32, 16, 3, &hi, D + nb) && ok(D, Q, C, P, 32, 16, 3, &hi, D - 48));  // touching
    for (uintptr_t b : {D, Q, C, P}) CHECK(!ok(D, Q, C, P, 32, 16, 3, &hi, b) && !ok(D, Q, C, P, 32, 16, 3, &hi, b + nb - 4) && !ok(D, Q, C, P, 32, 16, 3, &hi, b - 44));
    for (uintptr_t off : {1, 2, 3}) CHECK(!ok(D, Q, C, P, 32, 16, 3, &hi, S + off));
    printf("deinterlace: %d frames at 8 sizes x 8 parameter sets with and without a previous frame, out of place and in place, scalar and range checks\n", frames);
}

// the thumbnail and the block rule restated cell by cell: every cell looks its own block up
static void ref_scenecut(std::vector<uint8_t> &thumb, const uint8_t *cur, const uint8_t *tprev, int w, int h, const h264mi_scenecut &p, uint32_t *st) {
    const int tw = (w + 3) / 4, th = (h + 3) / 4, nbx = (tw + 7) / 8, nby = (th + 7) / 8;
    std::vector<long long> sad((size_t)nbx * nby, 0), sc(sad), sp(sad), nc(sad);
    for (int cy = 0; cy < th; cy++)
        for (int cx = 0; cx < tw; cx++) {
            long long sum = 0, n = 0;
            for (int y = 4 * cy; y < std::min(4 * cy + 4, h); y++)
                for (int x = 4 * cx; x < std::min(4 * cx + 4, w); x++) { sum += cur[(size_t)y * w + x]; n++; }
            const long long T = (sum + n / 2) / n, P = tprev[(size_t)cy * tw + cx];
            const size_t b = (size_t)(cy / 8) * nbx + cx / 8;
            thumb[(size_t)cy * tw + cx] = (uint8_t)T;
            sad[b] += llabs(T - P); sc[b] += T; sp[b] += P; nc[b]++;
        }
    for (int k = 0; k < 8; k++) st[k] = 0;
    for (size_t b = 0; b < sad.size(); b++) {
        const long long m = p.compensate ? sad[b] - llabs(sc[b] - sp[b]) : sad[b];
        st[0] += 4 * m > (long long)p.level * nc[b];
        st[1]++;
        st[2] += (uint32_t)sad[b]; st[3] += (uint32_t)sc[b]; st[4] += (uint32_t)sp[b];
    }
}

static void check_scenecut() {
    const int sizes[][2] = {{2, 2}, {6, 2}, {34, 18}, {66, 34}, {130, 70}, {514, 34}, {48, 66}};
    const h264mi_scenecut sets[] = {{64, 128, 4, 0, 1}, {64, 128, 4, 0, 0}, {0, 1, 0, 0, 1}, {1020, 256, 0, 9, 0}, {24, 64, 0, 0, 1}};
    int frames = 0;
    for (const auto &s : sizes)
        for (const h264mi_scenecut &p : sets) {
            const int w = s[0], h = s[1];
            const size_t fb = i420_bytes(w, h), tb = thumb_bytes(w, h);
            CHECK(tb == (size_t)((w + 3) / 4) * ((h + 3) / 4));
            std::unique_ptr<uint8_t[]> cur(new uint8_t[fb]), tp(new uint8_t[tb]), out(new uint8_t[tb]);  // exactly the bytes
            for (size_t i = 0; i < fb; i++) cur[i] = (uint8_t)pix_rng();
            for (size_t i = 0; i < tb; i++) tp[i] = (i / 3) % 2 ? (uint8_t)pix_rng() : (uint8_t)(120 + pix_rng() % 16);
            std::vector<uint8_t> want(tb);
            uint32_t st_want[8], st[8] = {9, 9, 9, 9, 9, 9, 9, 9};
            ref_scenecut(want, cur.get(), tp.get(), w, h, p, st_want);
            scenecut_frame_host(st, out.get(), cur.get(), tp.get(), w, h, p);
            CHECK(memcmp(out.get(), want.data(), tb) == 0 && memcmp(st, st_want, sizeof st) == 0);
            CHECK(st[0] <= st[1] && st[5] == 0 && st[6] == 0 && st[7] == 0);
            uint32_t st2[8] = {9, 9, 9, 9, 9, 9, 9, 9};
            scenecut_frame_host(st2, nullptr, cur.get(), tp.get(), w, h, p);  // statistics only
            CHECK(memcmp(st2, st_want, sizeof st2) == 0);
            memset(out.get(), 0, tb);
            scenecut_frame_host(nullptr, out.get(), cur.get(), nullptr, w, h, p);  // thumbnails only
            CHECK(memcmp(out.get(), want.data(), tb) == 0);
            scenecut_frame_host(st2, tp.get(), cur.get(), tp.get(), w, h, p);  // in place over the previous thumbnail
            CHECK(memcmp(tp.get(), want.data(), tb) == 0 && memcmp(st2, st_want, sizeof st2) == 0);
            frames++;
        }
    // the cut test at its boundary and at the largest counts; the scalar checks at their limits and one past each
    CHECK(!scenecut_is_cut(128, 4, 8) && scenecut_is_cut(128, 5, 8) && !scenecut_is_cut(0, 8, 8) && !scenecut_is_cut(256, 65536, 65536));
    CHECK(scenecut_is_cut(255, 65536, 65536) && scenecut_is_cut(1, 1, 255) && !scenecut_is_cut(1, 1, 256));
    const h264mi_scenecut lo{0, 0, 0, 0, 0}, hi{1020, 256, 65535, 65535, 1};
    CHECK(scenecut_ok(&lo) && scenecut_ok(&hi) && !scenecut_ok(nullptr));
    for (int f = 0; f < 5; f++) {
        h264mi_scenecut a = lo, b = hi;
        ((int32_t *)&a)[f]--; ((int32_t *)&b)[f]++;
        CHECK(!scenecut_ok(&a) && !scenecut_ok(&b));
        a = lo; ((int32_t *)&a)[f] = INT32_MIN; b = hi; ((int32_t *)&b)[f] = INT32_MAX;
        CHECK(!scenecut_ok(&a) && !scenecut_ok(&b));
    }
    const uintptr_t S = 0x10000000u, O = 0x20000000u, C = 0x30000000u, P = 0x40000000u;
    auto ok = [&](uintptr_t s, uintptr_t o, uintptr_t c, uintptr_t q, int w, int h, int n, const h264mi_scenecut *par) {
        return scenecut_args_ok((const void *)s, (const void *)o, (const void *)c, (const void *)q, w, h, n, par);
    };
    const size_t fb = 3 * i420_bytes(32, 16), tb = 3 * thumb_bytes(32, 16), sb = 96;
    CHECK(ok(S, O, C, P, 32, 16, 3, &hi) && ok(S, P, C, P, 32, 16, 3, &hi) && ok(S, 0, C, P, 32, 16, 3, &hi) && ok(0, O, C, 0, 32, 16, 3, &hi));
    CHECK(ok(0, O, C, P, 32, 16, 3, &hi) && ok(S, O, C, P, 8192, 8192, 1, &lo) && ok(0, O, C, 0, 2, 2, 1, &lo));
    CHECK(!ok(S, O, 0, P, 32, 16, 3, &hi) && !ok(0, 0, C, P, 32, 16, 3, &hi) && !ok(S, O, C, 0, 32, 16, 3, &hi) && !ok(S, O, C, P, 32, 16, 3, nullptr));
    CHECK(!ok(S, O, C, P, 32, 16, 0, &hi) && !ok(S, O, C, P, 31, 16, 3, &hi) && !ok(S, O, C, P, 32, 8194, 3, &hi) && !ok(S, O, C, P, 0, 16, 3, &hi));
    for (uintptr_t off : {(uintptr_t)1, (uintptr_t)(tb - 1), (uintptr_t)-1, (uintptr_t)-(intptr_t)(tb - 1)}) CHECK(!ok(S, P + off, C, P, 32, 16, 3, &hi));
    for (uintptr_t off : {(uintptr_t)0, (uintptr_t)(fb - 1), (uintptr_t)-(intptr_t)(tb - 1)})
        CHECK(!ok(S, C + off, C, P, 32, 16, 3, &hi) && !ok(S, O, C, C + off, 32, 16, 3, &hi));
    CHECK(ok(S, C + fb, C, P, 32, 16, 3, &hi) && ok(S, C - tb, C, P, 32, 16, 3, &hi) && ok(C + fb, O, C, P, 32, 16, 3, &hi) && ok(C - sb, O, C, P, 32, 16, 3, &hi));  // touching
    CHECK(!ok(C, O, C, P, 32, 16, 3, &hi) && !ok(C + fb - 4, O, C, P, 32, 16, 3, &hi) && !ok(C - sb + 4, O, C, P, 32, 16, 3, &hi));
    for (uintptr_t b : {O, P}) CHECK(!ok(b, O, C, P, 32, 16, 3, &hi) && !ok(b + tb - 4, O, C, P, 32, 16, 3, &hi) && !ok(b - sb + 4, O, C, P, 32, 16, 3, &hi));
    for (uintptr_t off : {1, 2, 3}) CHECK(!ok(S + off, O, C, P, 32, 16, 3, &hi));
    printf("scenecut: %d frames at 7 sizes x 5 parameter sets (with and without outputs, in place), the cut test, scalar and range checks\n", frames);
}

// the filter restated the other way round: columns first into a 32-bit plane, then rows; the rule spelt out again
static void ref_spatial(std::vector<uint8_t> &out, const uint8_t *src, int w, int h, const h264mi_spatial &p) {
    static const int W[4][7] = {{1}, {1, 2, 1}, {1, 4, 6, 4, 1}, {1, 6, 15, 20, 15, 6, 1}};
    size_t off = 0;
    for (int pl = 0; pl < 3; pl++) {
        const int pw = pl ? w / 2 : w, ph = pl ? h / 2 : h, r = pl ? p.radius_c : p.radius_y, am = pl ? p.amount_c : p.amount_y;
        std::vector<long long> v((size_t)pw * ph);
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                long long s = 0;
                for (int j = -r; j <= r; j++) s += (long long)W[r][j + r] * src[off + (size_t)std::min(std::max(y + j, 0), ph - 1) * pw + x];
                v[(size_t)y * pw + x] = s;
            }
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                long long s = 0;
                for (int i = -r; i <= r; i++) s += (long long)W[r][i + r] * v[(size_t)y * pw + std::min(std::max(x + i, 0), pw - 1)];
                const long long c = src[off + (size_t)y * pw + x];
                long long o = c;
                if (r > 0) {
                    const long long l = (s + (1ll << (4 * r - 1))) >> (4 * r), d = c - l;
                    if (!(am > 0 && llabs(d) <= p.core)) {
                        const long long t = am * d + 32;
                        o = c + (t >= 0 ? t / 64 : -((-t + 63) / 64));  // the floor without a shift
                        o = std::min(255ll, std::max(0ll, o));
                    }
                }
                out[off + (size_t)y * pw + x] = (uint8_t)o;
            }
        off += (size_t)pw * ph;
    }
}
// the masks restated per sample: every sample looks up its rectangle and its cell
static void ref_privacy(std::vector<uint8_t> &fr, int w, int h, int nframes, const std::vector<h264mi_privacy> &list) {
    const std::vector<uint8_t> src(fr);
    const size_t fb = i420_bytes(w, h);
    for (int f = 0; f < nframes; f++) {
        size_t off = 0;
        for (int pl = 0; pl < 3; pl++) {
            const int sh = pl ? 1 : 0, pw = w >> sh, ph = h >> sh;
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++)
                    for (const h264mi_privacy &m : list) {
                        const int rx = m.x >> sh, ry = m.y >> sh, rw = m.w >> sh, rh = m.h >> sh;
                        if (m.frame != f || x < rx || x >= rx + rw || y < ry || y >= ry + rh) continue;
                        uint8_t *o = &fr[f * fb + off + (size_t)y * pw + x];
                        if (m.mode == H264MI_PRIVACY_FILL) { *o = (uint8_t)(pl == 0 ? m.fill_y : pl == 1 ? m.fill_cb : m.fill_cr); continue; }
                        const int B = m.block >> sh, x0 = rx + (x - rx) / B * B, y0 = ry + (y - ry) / B * B;
                        const int x1 = std::min(x0 + B, rx + rw), y1 = std::min(y0 + B, ry + rh);
                        long long sum = 0, n = 0;
                        for (int yy = y0; yy < y1; yy++)
                            for (int xx = x0; xx < x1; xx++) { sum += src[f * fb + off + (size_t)yy * pw + xx]; n++; }
                        *o = (uint8_t)((sum + n / 2) / n);
                    }
            off += (size_t)pw * ph;
        }
    }
}

static void check_spatial() {
    const int sizes[][2] = {{2, 2}, {4, 4}, {8, 6}, {16, 16}, {36, 18}, {130, 66}, {260, 34}};
    const h264mi_spatial sets[] = {{1, 2, 40, -17, 3}, {2, 3, -64, 255, 0}, {3, 1, 255, -64, 0}, {3, 3, -17, 40, 255}, {0, 2, 40, 40, 3},
                                   {2, 0, -64, 40, 0}, {1, 1, 0, 0, 0}, {3, 3, 255, 255, 0}};
    int frames = 0;
    for (const auto &s : sizes)
        for (const h264mi_spatial &p : sets) {
            const int w = s[0], h = s[1];
            const size_t fb = i420_bytes(w, h);
            std::unique_ptr<uint8_t[]> src(new uint8_t[fb]), out(new uint8_t[fb]);  // exactly the frame's bytes
            for (size_t i = 0; i < fb; i++) src[i] = (i / 5) % 3 == 0 ? (uint8_t)(255 * ((i / 2) & 1)) : (i / 7) % 4 == 0 ? 90 : (uint8_t)pix_rng();
            memset(out.get(), 0x5A, fb);
            std::vector<uint8_t> want(fb);
            ref_spatial(want, src.get(), w, h, p);
            spatial_frame_host(out.get(), src.get(), w, h, p);
            CHECK(memcmp(out.get(), want.data(), fb) == 0);
            if (spatial_inert(p)) CHECK(memcmp(out.get(), src.get(), fb) == 0);
            frames++;
        }
    for (int r = 1; r <= 3; r++) {
        int sum = 0;
        for (int k = 0; k <= 2 * r; k++) { sum += spatial_weight(r, k); CHECK(spatial_weight(r, k) == spatial_weight(r, 2 * r - k)); }
        CHECK(sum == 1 << (2 * r));
    }
    CHECK(spatial_sample(100, 90, 64, 0) == 110 && spatial_sample(100, 90, -64, 0) == 90 && spatial_sample(100, 97, 255, 3) == 100);
    CHECK(spatial_sample(100, 97, -17, 3) == 99 && spatial_sample(250, 0, 255, 0) == 255 && spatial_sample(5, 255, 255, 0) == 0);
    // the masks on heap blocks of exactly the frames' bytes
    const int w = 130, h = 66, nf = 3;
    const std::vector<std::vector<h264mi_privacy>> lists = {
        {{0, 2, 4, 126, 58, 0, 4, 0, 0, 0}},
        {{1, 0, 0, 130, 66, 0, 64, 0, 0, 0}, {2, 0, 0, 130, 66, 0, 4, 0, 0, 0}, {0, 128, 64, 2, 2, 0, 4, 0, 0, 0}},
        {{0, 0, 0, 64, 32, 0, 8, 0, 0, 0}, {0, 64, 32, 66, 34, 0, 32, 0, 0, 0}, {1, 32, 16, 16, 16, 0, 16, 0, 0, 0}, {2, 6, 2, 100, 50, 1, 0, 17, 200, 90},
         {1, 100, 40, 30, 26, 1, 0, 0, 255, 128}},
    };
    int nlists = 0;
    for (const auto &list : lists) {
        const size_t nb = nf * i420_bytes(w, h);
        std::unique_ptr<uint8_t[]> fr(new uint8_t[nb]);
        std::unique_ptr<h264mi_privacy[]> hl(new h264mi_privacy[list.size()]);  // exactly the entries
        for (size_t k = 0; k < list.size(); k++) hl[k] = list[k];
        std::vector<uint8_t> want(nb);
        for (size_t i = 0; i < nb; i++) want[i] = fr[i] = (uint8_t)pix_rng();
        CHECK(privacy_ok(hl.get(), (int)list.size(), w, h, nf));
        ref_privacy(want, w, h, nf, list);
        privacy_frames_host(fr.get(), w, h, hl.get(), (int)list.size());
        CHECK(memcmp(fr.get(), want.data(), nb) == 0);
        nlists++;
    }
    // the scalar checks at their limits and one past each
    const h264mi_spatial lo{0, 0, -64, -64, 0}, hi{3, 3, 255, 255, 255};
    CHECK(spatial_ok(&lo) && spatial_ok(&hi) && !spatial_ok(nullptr));
    for (int f = 0; f < 5; f++) {
        h264mi_spatial a = lo, b = hi;
        ((int32_t *)&a)[f]--; ((int32_t *)&b)[f]++;
        CHECK(!spatial_ok(&a) && !spatial_ok(&b));
        a = lo; ((int32_t *)&a)[f] = INT32_MIN; b = hi; ((int32_t *)&b)[f] = INT32_MAX;
        CHECK(!spatial_ok(&a) && !spatial_ok(&b));
    }
    const uintptr_t D = 0x10000000u, S = 0x20000000u;
    auto ok = [&](uintptr_t d, uintptr_t s, int ww, int hh, int n, const h264mi_spatial *par) {
        return spatial_args_ok((const void *)d, (const void *)s, ww, hh, n, par);
    };
    const size_t nb = 3 * i420_bytes(32, 16);
    CHECK(ok(D, S, 32, 16, 3, &hi) && ok(D, S, 8192, 8192, 1, &lo) && ok(D, S, 2, 2, 1, &lo) && ok(D, D + nb, 32, 16, 3, &hi) && ok(D, D - nb, 32, 16, 3, &hi));
    CHECK(!ok(0, S, 32, 16, 3, &hi) && !ok(D, 0, 32, 16, 3, &hi) && !ok(D, S, 32, 16, 3, nullptr) && !ok(D, S, 32, 16, 0, &hi) && !ok(D, S, 32, 16, -1, &hi));
    CHECK(!ok(D, S, 31, 16, 3, &hi) && !ok(D, S, 32, 15, 3, &hi) && !ok(D, S, 0, 16, 3, &hi) && !ok(D, S, 8194, 16, 3, &hi) && !ok(D, S, 32, 8194, 3, &hi));
    for (uintptr_t off : {(uintptr_t)0, (uintptr_t)1, (uintptr_t)(nb - 1), (uintptr_t)-1, (uintptr_t)-(intptr_t)(nb - 1)}) CHECK(!ok(D, D + off, 32, 16, 3, &hi));
    auto one = [&](h264mi_privacy m, int ww = 32, int hh = 16, int nfr = 2) {
        std::unique_ptr<h264mi_privacy[]> q(new h264mi_privacy[1]);
        q[0] = m;
        return privacy_ok(q.get(), 1, ww, hh, nfr);
    };
    const h264mi_privacy g{1, 28, 12, 4, 4, 0, 4, 0, 0, 0}, fl{0, 0, 0, 32, 16, 1, 0, 255, 255, 255};
    CHECK(one(g) && one(fl) && one({0, 30, 14, 2, 2, 0, 64, -9, 999, 0}) && one({0, 0, 0, 2, 2, 1, 77, 0, 0, 0}));
    CHECK(!one(g, 32, 16, 1) && !one(g, 31, 16) && !one(g, 32, 8194) && !one(g, 30, 16) && !one(g, 32, 14) && !one(g, 32, 16, 0));
    for (int f = 0; f < 5; f++) {  // frame, x, y, w, h: one below, one past, odd, and the extremes
        h264mi_privacy a = g, b = g, c = g, d = g;
        ((int32_t *)&a)[f] = f == 0 ? -1 : f < 3 ? -2 : 0;
        ((int32_t *)&b)[f] += f == 0 ? 1 : 2;
        ((int32_t *)&c)[f] = INT32_MAX - (f > 0);
        ((int32_t *)&d)[f] = INT32_MIN;
        CHECK(!one(a) && !one(b) && !one(c) && !one(d));
        if (f > 0) { h264mi_privacy o = g; ((int32_t *)&o)[f]--; CHECK(!one(o)); }
    }
    for (int blk : {0, 2, 3, 5, 6, 12, 63, 65, 128, -4, INT32_MAX, INT32_MIN}) { h264mi_privacy a = g; a.block = blk; CHECK(!one(a)); }
    for (int blk : {4, 8, 16, 32, 64}) { h264mi_privacy a = g; a.block = blk; CHECK(one(a)); }
    for (int mode : {-1, 2, INT32_MAX, INT32_MIN}) { h264mi_privacy a = g; a.mode = mode; CHECK(!one(a)); }
    for (int f = 7; f < 10; f++) {
        h264mi_privacy a = fl, b = fl;
        ((int32_t *)&a)[f] = 256; ((int32_t *)&b)[f] = -1;
        CHECK(!one(a) && !one(b));
    }
    {   // two entries: touching, sharing one sample, the same rectangle on two frames; the counts
        std::unique_ptr<h264mi_privacy[]> q(new h264mi_privacy[2]);
        q[0] = {0, 0, 0, 16, 8, 0, 8, 0, 0, 0}; q[1] = {0, 16, 0, 16, 8, 1, 0, 1, 2, 3};
        CHECK(privacy_ok(q.get(), 2, 32, 16, 2));
        q[1].x = 14; CHECK(!privacy_ok(q.get(), 2, 32, 16, 2));
        q[1].frame = 1; CHECK(privacy_ok(q.get(), 2, 32, 16, 2));
        CHECK(!privacy_ok(q.get(), 0, 32, 16, 2) && !privacy_ok(q.get(), -1, 32, 16, 2) && !privacy_ok(nullptr, 2, 32, 16, 2));
        std::unique_ptr<h264mi_privacy[]> many(new h264mi_privacy[PIC_MAX_LIST]);
        for (int k = 0; k < PIC_MAX_LIST; k++) many[k] = {0, 2 * k, 0, 2, 2, 1, 0, 1, 2, 3};
        CHECK(privacy_ok(many.get(), PIC_MAX_LIST, 8192, 2, 1) && !privacy_ok(many.get(), PIC_MAX_LIST + 1, 8192, 2, 1));
    }
    printf("spatial: %d frames at 7 sizes x 8 parameter sets, the weights and the sample rule; privacy: %d lists on 3 frames of 130x66; scalar, list and range checks\n",
           frames, nlists);
}

// ---- levels.hip's host restatements against a second statement of the rules: counts by sorting the samples, the ends
// from sums taken afresh for every bin in 64 bits, the table entries in 64 bits with the division written as a search
static void check_levels() {
    const int sizes[6][2] = {{2, 2}, {4, 4}, {16, 16}, {36, 18}, {130, 66}, {64, 48}};
    const h264mi_levels sets[8] = {{0, 0, 0, 0, 0, 0, 255, 1024, 256, 64},  {0, 0, 0, 0, 0, 16, 235, 64, 256, 64},  {0, 2048, 2048, 0, 0, 16, 235, 256, 37, 64},
                                   {0, 4096, 4096, 0, 0, 0, 255, 1024, 37, 0}, {0, 0, 4096, 0, 0, 0, 255, 64, 255, 80}, {0, 4096, 0, 0, 0, 0, 1, 1024, 1, 255},
                                   {1, 0, 0, 16, 235, 0, 255, 64, 1, 64},    {1, 4096, 4096, 100, 101, 0, 255, 1024, 256, 255}};
    uint32_t seed = 99;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    int frames = 0;
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1];
        const size_t nb = i420_bytes(w, h), ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
        for (int content = 0; content < 3; content++) {
            std::unique_ptr<uint8_t[]> src(new uint8_t[nb]), out(new uint8_t[nb]), want(new uint8_t[nb]);
            for (size_t i = 0; i < nb; i++) src[i] = content == 0 ? (uint8_t)rnd() : content == 1 ? (uint8_t)(20 + rnd() % 41) : (uint8_t)(i < ly / 32 ? 0 : i + ly / 32 + 1 >= ly && i < ly ? 255 : 77);
            std::unique_ptr<uint32_t[]> hist(new uint32_t[768]);
            hist_frame_host(hist.get(), src.get(), w, h);
            const size_t len[3] = {ly, lc, lc};
            size_t at = 0;
            for (int pl = 0; pl < 3; at += len[pl], pl++) {
                std::vector<uint8_t> sorted(src.get() + at, src.get() + at + len[pl]);
                std::sort(sorted.begin(), sorted.end());
                for (int v = 0; v < 256; v++)
                    CHECK(hist[256 * pl + v] == (uint32_t)(std::upper_bound(sorted.begin(), sorted.end(), (uint8_t)v) - std::lower_bound(sorted.begin(), sorted.end(), (uint8_t)v)));
            }
            std::unique_ptr<int32_t[]> state(new int32_t[4]), rec(new int32_t[8]);
            std::unique_ptr<uint8_t[]> lut(new uint8_t[768]);
            for (const auto &p : sets) {
                CHECK(levels_ok(&p));
                for (int pass = 0; pass < 3; pass++) {  // no state, a first frame, a later frame
                    const int32_t st0[4] = {pass == 2 ? 1 : 0, 31 * 256 + 7, 200 * 256 - 9, 5};
                    memcpy(state.get(), st0, sizeof st0);
                    levels_lut_host(lut.get(), p.mode == H264MI_LEVELS_AUTO ? hist.get() : nullptr, w, h, p, pass ? state.get() : nullptr, rec.get());
                    int64_t lo_e, hi_e;
                    if (p.mode == H264MI_LEVELS_FIXED) {
                        lo_e = 256 * (int64_t)p.in_lo; hi_e = 256 * (int64_t)p.in_hi;
                        CHECK(rec[0] == 0 && rec[1] == 0 && rec[2] == 0 && rec[3] == 0 && rec[6] == 0 && rec[7] == 0);
                        CHECK(!pass || memcmp(state.get(), st0, sizeof st0) == 0);
                    } else {
                        const int64_t npix = (int64_t)w * h, k_lo = p.clip_lo * npix / 65536, k_hi = p.clip_hi * npix / 65536;
                        int lo_m = -1, hi_m = -1;
                        for (int v = 0; v < 256; v++) {
                            int64_t le = 0, ge = 0;
                            for (int u = 0; u <= v; u++) le += hist[u];
                            for (int u = v; u < 256; u++) ge += hist[u];
                            if (le > k_lo && lo_m < 0) lo_m = v;
                            if (ge > k_hi) hi_m = v;
                        }
                        CHECK(lo_m >= 0 && lo_m <= hi_m && rec[0] == lo_m && rec[1] == hi_m);
                        int64_t lo_s = 256 * lo_m, hi_s = 256 * hi_m;
                        if (pass == 2) {
                            auto floor_div = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
                            lo_s = st0[1] + floor_div((256 * (int64_t)lo_m - st0[1]) * p.speed, 256);
                            hi_s = st0[2] + floor_div((256 * (int64_t)hi_m - st0[2]) * p.speed, 256);
                        }
                        CHECK(rec[2] == lo_s && rec[3] == hi_s);
                        if (pass) CHECK(state[0] == 1 && state[1] == lo_s && state[2] == hi_s && state[3] == 0);
                        const int64_t R = p.out_hi - p.out_lo, min_span = std::max<int64_t>(16, R * 16384 / p.max_gain);
                        lo_e = lo_s; hi_e = hi_s;
                        if (hi_s - lo_s < min_span) {
                            const int64_t sum = lo_s + hi_s - min_span;
                            lo_e = sum >= 0 ? sum / 2 : -((-sum + 1) / 2);
                            hi_e = lo_e + min_span;
                        }
                        int64_t below = 0, above = 0;
                        for (int v = 0; v < 256; v++) { below += 256 * v < lo_e ? hist[v] : 0; above += 256 * v > hi_e ? hist[v] : 0; }
                        CHECK(rec[6] == below && rec[7] == above);
                    }
                    CHECK(rec[4] == lo_e && rec[5] == hi_e && hi_e - lo_e >= 16);
                    const int64_t R = p.out_hi - p.out_lo, span = hi_e - lo_e;
                    for (int v = 0; v < 256; v++) {
                        const int64_t t = 256 * v - lo_e;
                        int64_t y = p.out_lo;
                        if (t > 0) {
                            int64_t q = 0;  // the largest q with q span <= t R + span / 2
                            while ((q + 1) * span <= t * R + span / 2 && q < R) q++;
                            y = p.out_lo + q;
                        }
                        CHECK(lut[v] == y);
                        const int64_t g = (int64_t)(v - 128) * p.sat + 32, c = 128 + (g >= 0 ? g / 64 : -((-g + 63) / 64));
                        CHECK(lut[256 + v] == std::min<int64_t>(255, std::max<int64_t>(0, c)) && lut[512 + v] == lut[256 + v]);
                    }
                    lut_frame_host(out.get(), src.get(), w, h, lut.get());
                    at = 0;
                    for (int pl = 0; pl < 3; at += len[pl], pl++)
                        for (size_t i = 0; i < len[pl]; i++) want[at + i] = lut[256 * pl + src[at + i]];
                    CHECK(memcmp(out.get(), want.get(), nb) == 0);
                    memcpy(out.get(), src.get(), nb);
                    lut_frame_host(out.get(), out.get(), w, h, lut.get());  // in place
                    CHECK(memcmp(out.get(), want.get(), nb) == 0);
                }
            }
            frames++;
        }
    }
    // the ok-function one past every limit, the clip counts at the limit, the calls' argument checks
    const h264mi_levels good = {0, 100, 100, 10, 20, 16, 235, 256, 37, 64};
    CHECK(levels_ok(&good) && !levels_ok(nullptr) && !levels_inert(good));
    const int lim[9][2] = {{0, 4096}, {0, 4096}, {0, 255}, {0, 255}, {0, 255}, {0, 255}, {64, 1024}, {1, 256}, {0, 255}};
    for (int k = 0; k < 9; k++)
        for (int e = 0; e < 2; e++) {
            h264mi_levels b = good;
            (&b.clip_lo)[k] = lim[k][e] + (e ? 1 : -1);
            CHECK(!levels_ok(&b));
        }
    { h264mi_levels b = good; b.mode = 2; CHECK(!levels_ok(&b)); b.mode = -1; CHECK(!levels_ok(&b)); }
    { h264mi_levels b = good; b.out_hi = b.out_lo; CHECK(!levels_ok(&b)); b.mode = 1; b.out_hi = 235; b.in_hi = b.in_lo; CHECK(!levels_ok(&b)); b.in_hi = b.in_lo + 1; CHECK(levels_ok(&b)); }
    { h264mi_levels b = {1, 7, 7, 16, 235, 16, 235, 99, 9, 64}; CHECK(levels_ok(&b) && levels_inert(b)); b.sat = 65; CHECK(!levels_inert(b)); }
    CHECK(levels_clip_count(4096, 8192, 8192) == (1u << 22) && levels_clip_count(0, 8192, 8192) == 0 && levels_clip_count(4096, 2, 2) == 0 && levels_clip_count(4096, 4, 4) == 1);
    CHECK(levels_work_bytes(1) == 3840 && levels_work_bytes(128) == 128 * 3840);
    alignas(16) static uint8_t arena[1 << 16];
    uint8_t *A = arena;
    const size_t fb = i420_bytes(32, 16);
    CHECK(hist_args_ok(A, A + 8192, 32, 16, 2) && !hist_args_ok(A + 1, A + 8192, 32, 16, 2) && !hist_args_ok(A, A + 6140, 32, 16, 2) && hist_args_ok(A, A + 6144, 32, 16, 2));
    CHECK(!hist_args_ok(nullptr, A, 32, 16, 1) && !hist_args_ok(A, nullptr, 32, 16, 1) && !hist_args_ok(A, A + 8192, 32, 16, 0) && !hist_args_ok(A, A + 8192, 31, 16, 1));
    CHECK(lut_args_ok(A, A, 32, 16, 2, A + 8192, 1) && lut_args_ok(A, A + 2 * fb, 32, 16, 2, A + 8192, 0) && !lut_args_ok(A, A + 1, 32, 16, 2, A + 8192, 1));
    CHECK(!lut_args_ok(A, A, 32, 16, 2, A + 2 * fb - 1, 0) && lut_args_ok(A, A, 32, 16, 2, A + 2 * fb, 0) && !lut_args_ok(A + 767, A + 8192, 32, 16, 1, A, 1));
    CHECK(lut_args_ok(A + 768, A + 8192, 32, 16, 1, A, 0) && !lut_args_ok(A + 768, A + 8192, 32, 16, 1, A, 2) && !lut_args_ok(A, A, 32, 16, 2, nullptr, 0));
    uint8_t *W = A + 16384, *S = A + 32768, *Rc = A + 40960;
    CHECK(levels_args_ok(A, A, 32, 16, 2, &good, S, Rc, W) && levels_args_ok(A, A + 2 * fb, 32, 16, 2, &good, nullptr, nullptr, W));
    CHECK(!levels_args_ok(A, A + 4, 32, 16, 2, &good, S, Rc, W) && !levels_args_ok(A, A, 32, 16, 2, &good, S + 2, Rc, W) && !levels_args_ok(A, A, 32, 16, 2, &good, S, Rc + 1, W));
    CHECK(!levels_args_ok(A, A, 32, 16, 2, &good, S, Rc, W + 3) && !levels_args_ok(A, A, 32, 16, 2, &good, S, Rc, nullptr) && !levels_args_ok(A, A, 32, 16, 2, nullptr, S, Rc, W));
    CHECK(!levels_args_ok(A, A, 32, 16, 2, &good, S, S + 28, W) && levels_args_ok(A, A, 32, 16, 2, &good, S, S + 32, W) && !levels_args_ok(A, A, 32, 16, 2, &good, W + 7676, Rc, W));
    CHECK(levels_args_ok(A, A, 32, 16, 2, &good, W + 7680, Rc, W) && !levels_args_ok(A, A, 32, 16, 2, &good, S, Rc, A + 2 * fb - 4) && !levels_args_ok(W, A, 32, 16, 2, &good, S, Rc, W));
    printf("levels: %d frames at 6 sizes x 8 parameter sets x (no state, first frame, later frame): histogram, decision, tables, lookup in place and out; ok-function, clip counts and argument checks\n", frames);
}

int main() {
    check_levels();
    check_spatial();
    check_deinterlace();
    check_scenecut();
    check_denoise();
    check_pix();
    check_pixdeep();
    check_orient();
    check_cells();
    check_tables();
    check_layouts();
    check_scalars();
    printf(failures ? "%d FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
