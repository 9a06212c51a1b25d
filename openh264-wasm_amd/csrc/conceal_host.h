// conceal_host.h -- the gap rule of slice-copy concealment, in one place: dec_conceal_kernel, the
// frame decision and the exported h264mi_conceal_gaps all call conceal_gaps() below. No HIP call and no allocation:
// tools/conceal_host_san.hip runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#ifndef H264MI_MAX_SLICES
#define H264MI_MAX_SLICES 32
#endif
#define H264MI_MAX_GAPS (H264MI_MAX_SLICES + 1)  // n disjoint slices leave at most n + 1 uncovered runs

#if defined(__HIPCC__) || defined(__CUDACC__)
#define H264MI_HD __host__ __device__
#else
#define H264MI_HD
#endif

namespace h264mi {

// A good slice: parsed to its stop bit (ok) with first < end <= total (first_mb_in_slice, one past its last MB).
H264MI_HD inline bool conceal_good(int total, int first, int end, int ok) { return ok != 0 && first >= 0 && first < end && end <= total; }

// The slices of one picture (in any order) -> the gaps the good ones leave, as triples {first, end, donor}:
// a gap is a maximal run [first, end) of MB addresses no good slice covers; its donor is the index of the good
// slice that ends where the gap begins, or, for a gap at address 0, of the one that begins where it ends (the
// synthetic P slice of the gap takes SliceQPY and the loop-filter parameters from it). Gaps come in address order.
// Returns the number of gaps (0: the good slices tile the picture exactly; at most max_gaps triples are written),
// or -1 (reject: no good slice, two good slices overlap, or a bad argument). A slice that is not good contributes
// nothing.
H264MI_HD inline int conceal_gaps(int total, int nsl, const int *first, const int *end, const int *ok, int *gaps, int max_gaps) {
    if (total <= 0 || nsl <= 0 || nsl > H264MI_MAX_SLICES || !first || !end || !ok || max_gaps < 0 || (max_gaps > 0 && !gaps)) return -1;
    uint32_t left = 0;  // good slices not yet placed
    for (int j = 0; j < nsl; j++)
        if (conceal_good(total, first[j], end[j], ok[j])) left |= 1u << j;
    if (!left) return -1;
    int next = 0, prev = -1, n = 0;
    while (left) {
        int k = -1;  // the good slice with the lowest first_mb
        for (int j = 0; j < nsl; j++)
            if (((left >> j) & 1u) && (k < 0 || first[j] < first[k])) k = j;
        if (first[k] < next) return -1;  // it begins inside the one before it
        if (first[k] > next) {
            if (n < max_gaps) { gaps[3 * n] = next; gaps[3 * n + 1] = first[k]; gaps[3 * n + 2] = prev >= 0 ? prev : k; }
            n++;
        }
        next = end[k];
        prev = k;
        left &= ~(1u << k);
    }
    if (next < total) {
        if (n < max_gaps) { gaps[3 * n] = next; gaps[3 * n + 1] = total; gaps[3 * n + 2] = prev; }
        n++;
    }
    return n;
}

// What a slice that failed may have left behind: the records of [first, end) and part of end's coefficients
// (dec_parse.inc writes a macroblock's levels before its record). The picture is concealed only if none of that
// lies inside a good slice, whose records would otherwise be in doubt; it lies in a gap, which dec_conceal_kernel
// rewrites. first / end / ok as above; end[j] of a failed slice is the MB it stopped at (>= first[j]).
H264MI_HD inline bool conceal_clean(int total, int nsl, const int *first, const int *end, const int *ok) {
    for (int j = 0; j < nsl; j++) {
        if (conceal_good(total, first[j], end[j], ok[j])) continue;
        const int lo = first[j], hi = (end[j] > lo ? end[j] : lo) + 1;
        for (int k = 0; k < nsl; k++)
            if (conceal_good(total, first[k], end[k], ok[k]) && first[k] < hi && lo < end[k]) return false;
    }
    return true;
}

}  // namespace h264mi
