// conceal_host_san.cc -- the gap rule of slice-copy concealment (csrc/conceal_host.h: conceal_gaps, conceal_clean, the
// functions dec_conceal_kernel calls) under AddressSanitizer and UBSan on the CPU. A program of its own: nothing is
// loaded into Python, no kernel is launched, no device is needed.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/conceal_host_san.cc
//       -o conceal_host_san && ./conceal_host_san tests/golden/conceal_tables.txt
//
// The file holds the directed tables of tests/test_conceal_host.py, one per line:
//   total nsl  first end ok (nsl times)  ngaps (-1: reject)  first end donor (ngaps times)
// Every array lives in a heap block of exactly the size the call may touch, so a read or write past it is the
// sanitizer's to see. Each table runs with room for every gap, for one gap fewer (the count must not change, the
// triple past the room must stay untouched) and for none; then the same slices rotated (the donors rotate with
// them). conceal_clean runs on every table and on each with one failed slice laid over a good one.
// Prints one line per table and "ok"; exits 1 at the first difference.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../openh264-wasm_amd/csrc/conceal_host.h"

using namespace h264mi;

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                           \
        }                                                         \
    } while (0)

static std::unique_ptr<int[]> heap(const std::vector<int> &v) {
    std::unique_ptr<int[]> p(new int[v.size()]);
    for (size_t k = 0; k < v.size(); k++) p[k] = v[k];
    return p;
}

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { printf("usage: conceal_host_san tables.txt\n"); return 2; }
    int total, nsl, tables = 0;
    while (fscanf(f, "%d %d", &total, &nsl) == 2) {
        std::vector<int> first(nsl), end(nsl), ok(nsl);
        for (int j = 0; j < nsl; j++)
            if (fscanf(f, "%d %d %d", &first[j], &end[j], &ok[j]) != 3) return 2;
        int want = 0;
        if (fscanf(f, "%d", &want) != 1) return 2;
        std::vector<int> gaps(3 * (want > 0 ? want : 0));
        for (size_t k = 0; k < gaps.size(); k++)
            if (fscanf(f, "%d", &gaps[k]) != 1) return 2;
        for (int rot = 0; rot < (nsl > 1 ? 2 : 1); rot++) {  // as given, then rotated by one
            std::vector<int> rf(nsl), re(nsl), ro(nsl);
            for (int j = 0; j < nsl; j++) { rf[(j + rot) % nsl] = first[j]; re[(j + rot) % nsl] = end[j]; ro[(j + rot) % nsl] = ok[j]; }
            const auto pf = heap(rf), pe = heap(re), po = heap(ro);
            const int room = want > 0 ? want : 0;
            for (int less = 0; less <= (room > 0 ? 1 : 0); less++) {
                std::unique_ptr<int[]> out(new int[3 * (room - less) + 1]);  // + 1: never a zero-size block
                for (int k = 0; k < 3 * (room - less); k++) out[k] = -7;
                CHECK(conceal_gaps(total, nsl, pf.get(), pe.get(), po.get(), out.get(), room - less) == want);
                for (int k = 0; k < 3 * (room - less); k++)
                    CHECK(out[k] == (k % 3 == 2 ? (gaps[k] + rot) % nsl : gaps[k]));
            }
            CHECK(conceal_gaps(total, nsl, pf.get(), pe.get(), po.get(), nullptr, 0) == want);
            // a table without failed slices is clean; a failed slice laid over the first good one is not
            bool any_failed = false;
            int good = -1;
            for (int j = 0; j < nsl; j++) {
                if (!conceal_good(total, rf[j], re[j], ro[j])) any_failed = true;
                else if (good < 0) good = j;
            }
            if (!any_failed) CHECK(conceal_clean(total, nsl, pf.get(), pe.get(), po.get()));
            if (good >= 0 && nsl < H264MI_MAX_SLICES) {
                std::vector<int> xf = rf, xe = re, xo = ro;
                xf.push_back(rf[good]); xe.push_back(rf[good]); xo.push_back(0);  // stopped in the good slice's first MB
                const auto qf = heap(xf), qe = heap(xe), qo = heap(xo);
                CHECK(!conceal_clean(total, nsl + 1, qf.get(), qe.get(), qo.get()));
                CHECK(conceal_gaps(total, nsl + 1, qf.get(), qe.get(), qo.get(), nullptr, 0) == want);  // it contributes nothing
            }
        }
        printf("table %d: %d MBs, %d slices -> %d\n", tables++, total, nsl, want);
    }
    fclose(f);
    // arguments
    const auto one = heap({0}), ten = heap({10}), yes = heap({1});
    int g[3] = {-7, -7, -7};
    CHECK(conceal_gaps(0, 1, one.get(), ten.get(), yes.get(), g, 1) == -1 && conceal_gaps(20, 0, one.get(), ten.get(), yes.get(), g, 1) == -1);
    CHECK(conceal_gaps(20, 33, one.get(), ten.get(), yes.get(), g, 1) == -1 && conceal_gaps(20, 1, nullptr, ten.get(), yes.get(), g, 1) == -1);
    CHECK(conceal_gaps(20, 1, one.get(), ten.get(), yes.get(), nullptr, 1) == -1 && conceal_gaps(20, 1, one.get(), ten.get(), yes.get(), g, -1) == -1);
    CHECK(g[0] == -7 && conceal_gaps(20, 1, one.get(), ten.get(), yes.get(), g, 1) == 1 && g[0] == 10 && g[1] == 20 && g[2] == 0);
    CHECK(tables > 0);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
