// dec_parse.inc -- decoder bitstream parse (gfx950): NAL split, emulation-prevention removal,
// SPS/PPS/slice header, CAVLC macroblock layer (7.3, 9.2) -> per-MB records (MbInfo + MbCoef) with
// motion vectors, intra modes and QP resolved.
//
// Replaces the parse half of ISVCDecoder::DecodeFrameNoDelay (openh264_wrapper.cpp:435). A slice is
// one serial CAVLC chain, so one wave per stream walks it, and the design goal is the shortest
// possible dependency chain per syntax element:
//   * only what the syntax itself depends on is computed here -- nnz contexts for coeff_token and
//     the running QP. Motion vectors (mvp + mvd) and Intra4x4 modes are resolved later by
//     dec_recon_kernel, whose MB-row wavefront already holds every neighbour they need;
//   * the chain runs on the SCALAR unit: all parse state is wave-uniform and lives in SGPRs (values
//     read from LDS are pulled in with readfirstlane);
//   * bits come from a 64-bit SGPR cache refilled one dword at a time from a 16 KiB LDS ring that
//     the whole wave fills cooperatively with emulation-prevention bytes already removed;
//   * VLC tables are 32-bit entries in constant memory read with uniform indices, i.e. scalar loads
//     through the scalar cache (vlc_tables.inc, ~10 KB);
//   * the macroblock record under construction is a VGPR (lane w holds dword w of its MbInfo),
//     filled with v_writelane; the left neighbour's record is kept the same way (v_readlane);
//   * decoded levels sit one per lane; run_before scatters them to their scan positions with
//     writelane and lanes 0..15 store the block with one coalesced 32-byte store.
// Parse output (the "raw" record, see h264mi_types.h): i4mode[] holds the Intra4x4 mode codes in
// decoding order (0xff = prev_intra4x4_pred_mode_flag, else rem_intra4x4_pred_mode), mv[] holds the
// mvd of each partition at the raster slot of its first 4x4 block.
namespace h264mi {

constexpr int RING_BYTES = 16384;  // refilled whenever the reader is within half a ring of the write head
constexpr uint32_t RING_WMASK = RING_BYTES / 4 - 1;
constexpr int MAX_NALS = 32;


DEV uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
template <class T> DEV GLOBAL T *uni_ptr(T *p) {  // wave-uniform global pointer (SGPR pair)
    uint64_t v = (uint64_t)p;
    return (GLOBAL T *)(((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v));
}
DEV uint32_t rdlane(int v, int l) { return (uint32_t)__builtin_amdgcn_readlane(v, l); }
extern "C" __device__ int h264mi_llvm_writelane(int, int, int) __asm("llvm.amdgcn.writelane.i32");
DEV int wrlane(uint32_t x, int l, int v) { return h264mi_llvm_writelane((int)x, l, v); }  // v_writelane_b32

// Global stores from a constant set of low lanes. `if (lane < 16) p[lane] = v` compiles to a vector
// compare whose result the scalar unit waits for (s_and_saveexec on the VCC a v_cmp just wrote): ~20
// cycles on the serial chain per store. Here the scalar unit writes the lane mask to EXEC itself. off:
// the lane's byte offset (a VGPR computed once); base: a wave-uniform pointer (SGPR pair). EXEC is
// restored inside the block; the stores are never read back by this wave.
DEV void st_i16_l16(GLOBAL void *base, uint32_t off, int v) {  // lanes 0..15, 2 bytes each (off = 2 * lane)
    uint64_t sv;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, 0xffff\n\ts_mov_b32 exec_hi, 0\n\t"
                 "global_store_short %1, %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(sv) : "v"(off), "v"(v), "s"(base) : "memory");
}
DEV void st_u32_l32(GLOBAL void *base, uint32_t off, int v) {  // lanes 0..31, 4 bytes each (off = 4 * lane)
    uint64_t sv;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, 0\n\t"
                 "global_store_dword %1, %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(sv) : "v"(off), "v"(v), "s"(base) : "memory");
}

// ---------------------------------------------------------------- RBSP ring (LDS)
struct Ring {
    GLOBAL const uint8_t *in;
    int in_pos, in_end;  // NAL payload bytes (EP present)
    uint32_t c1, c2;     // last two input bytes (EP detection carry)
    uint32_t written;    // RBSP bytes written so far
};
// cooperative: append RBSP bytes (EP bytes dropped) until `target` bytes have been written. RBSP
// byte p is stored at ring[p ^ 3], so a little-endian dword load yields the next 32 bits in
// bitstream order (gfx9 has no scalar byte swap; a v_perm would drag the reader onto the VALU).
#ifndef H264MI_FILL_CHUNKS
#define H264MI_FILL_CHUNKS 8
#endif
constexpr int FILL_CHUNKS = H264MI_FILL_CHUNKS;  // 64-byte chunks whose loads are in flight together (one memory wait per 512 B)
DEV void ring_fill(Ring &RS, uint8_t *ring, uint32_t target) {  // RS: LDS (keeps SGPRs free)
    const int lane = threadIdx.x;
    Ring R;
    R.in = uni_ptr((const uint8_t *)RS.in); R.in_pos = uni(RS.in_pos); R.in_end = uni(RS.in_end);
    R.c1 = uni(RS.c1); R.c2 = uni(RS.c2); R.written = uni(RS.written);
    while (R.written < target && R.in_pos < R.in_end) {
        int bv[FILL_CHUNKS];
#pragma unroll
        for (int k = 0; k < FILL_CHUNKS; k++) {  // all loads issued before the first use
            // clamped, unconditional load: a guarded one is an EXEC-masked region with its own
            // vmcnt(0), which serialises the batch (in_end > in_pos here)
            const int i = R.in_pos + 64 * k + lane;
            const int v = R.in[min(i, R.in_end - 1)];
            bv[k] = i < R.in_end ? v : 0xff;
        }
#pragma unroll
        for (int k = 0; k < FILL_CHUNKS; k++) {
            if (R.in_pos >= R.in_end || R.written >= target) break;  // overshoot stays < 64 bytes, as before
            const int b = bv[k];
            const bool valid = R.in_pos + lane < R.in_end;
            int p1 = __shfl_up(b, 1), p2 = __shfl_up(b, 2);
            if (lane == 0) { p1 = (int)R.c1; p2 = (int)R.c2; }
            if (lane == 1) p2 = (int)R.c1;
            const bool rm = valid && b == 3 && p1 == 0 && p2 == 0;
            const bool kept = valid && !rm;
            const uint64_t m = __ballot(kept);
            const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            if (kept) ring[((R.written + rank) ^ 3) & (RING_BYTES - 1)] = (uint8_t)b;  // byte-swapped per dword
            R.written += (uint32_t)__popcll(m);
            const int n = min(64, R.in_end - R.in_pos);
            R.c2 = n >= 2 ? uni((uint32_t)__shfl(b, n - 2)) : R.c1;
            R.c1 = uni((uint32_t)__shfl(b, n - 1));
            R.in_pos += 64;
        }
    }
    __syncthreads();
    if (lane == 0) RS = R;
    __syncthreads();
}
// ring dword index at which the reader must top the ring up again (~0u: input exhausted)
DEV uint32_t ring_refill_at(const Ring &RS) {
    if (uni(RS.in_pos) >= uni(RS.in_end)) return ~0u;
    const uint32_t w = uni(RS.written);
    return w > RING_BYTES / 2u ? (w - RING_BYTES / 2u) >> 2 : 0u;
}

// ---------------------------------------------------------------- scalar bit reader
struct Bits {
    const uint32_t *ring32;
    uint64_t cache;   // MSB-aligned
    int32_t avail;    // valid bits in cache
    uint32_t widx;    // next ring dword
    uint32_t err;
};
DEV void br_refill(Bits &b) {  // afterwards avail >= 32
    if (b.avail <= 32) {
        uint32_t w = uni(b.ring32[b.widx & RING_WMASK]);
        b.cache |= (uint64_t)w << (32 - b.avail);
        b.avail += 32;
        b.widx++;
    }
}
DEV uint32_t br_peek(const Bits &b) { uint32_t p = (uint32_t)(b.cache >> 32); asm("" : "+s"(p)); return p; }
DEV void br_skip(Bits &b, int n) { b.cache <<= n; b.avail -= n; }
DEV uint32_t br_pos(const Bits &b) { return b.widx * 32u - (uint32_t)b.avail; }
DEV void br_seek(Bits &b, uint32_t pos) {
    b.widx = pos >> 5; b.cache = 0; b.avail = 0;
    br_refill(b); br_refill(b);
    br_skip(b, (int)(pos & 31));
}
DEV uint32_t br_bits(Bits &b, int n) {  // 1..32 bits
    br_refill(b);
    uint32_t v = (uint32_t)(b.cache >> (64 - n));
    br_skip(b, n);
    return v;
}
DEV uint32_t br_ue(Bits &b) {
    br_refill(b);
    uint32_t p = br_peek(b);
    int lz = __clz(p);
    if (lz < 16) { br_skip(b, 2 * lz + 1); return (p >> (31 - 2 * lz)) - 1; }
    if (lz >= 32) { b.err = 1; return 0; }
    br_skip(b, lz);
    return br_bits(b, lz + 1) - 1;
}
DEV int br_se(Bits &b) {
    uint32_t k = br_ue(b);
    return (k & 1) ? (int)((k + 1) >> 1) : -(int)(k >> 1);
}

// ---------------------------------------------------------------- register bit reader (slice data)
// The slice-data chain reads its bits from two VGPR windows instead of LDS: w0 holds ring dwords
// wb .. wb+63 (lane l = dword wb+l), w1 the next 64. Pulling the next 32 bits into the SGPR cache is a
// v_readlane (~25 cycles on the chain) rather than an LDS read + readfirstlane (~116). The windows move
// only at macroblock boundaries (vr_slide, at the top of the macroblock loop, which is also where the
// LDS ring is topped up): once the reader is 16 dwords into w0 both windows are reloaded at wb = wi & ~15,
// so at least 112 dwords (3584 bits) lie ahead, which covers a conforming macroblock_layer() (7.4.5 /
// A.3.1: at most 128 + RawMbBits = 3200 bits) and its mb_skip_run; I_PCM re-seeks. A larger macroblock
// (escape-coded levels at low QP can exceed the conformance bound) is covered by vr_reslide before each
// luma 8x8 quarter, the I16 DC block, the chroma DC pair and each chroma AC plane: a reload when the reader
// is 40 dwords into w0 (>= 88 dwords, 2816 bits, ahead: more than four 4x4 blocks of <= 638 bits). The ring
// holds >= 8 KiB beyond the reader at every macroblock top, so these reloads never need a ring fill. In the
// common case w0 / w1 do not change inside a macroblock: no window copies and no LDS waits on the chain.
struct VR {
    uint64_t c;    // MSB-aligned cache
    int32_t n;     // valid bits in c
    uint32_t wi;   // next ring dword to pull into the cache
    uint32_t wb;   // ring dword held by lane 0 of w0
    int w0, w1;    // VGPR windows
    uint32_t err;
};
DEV void vr_fill(VR &r) {  // afterwards n >= 33
    if (r.n <= 32) {
        const uint32_t s = r.wi - r.wb;
        const uint32_t a = rdlane(r.w0, (int)(s & 63)), b = rdlane(r.w1, (int)(s & 63));
        r.c |= (uint64_t)(s < 64 ? a : b) << (32 - r.n);
        r.n += 32;
        r.wi++;
    }
}
// opaque to the optimiser: otherwise tests on clz(peek) become 64-bit compares of the cache, which
// gfx9 can only do on the VALU (a VALU -> VCC -> branch round trip on the chain)
DEV uint32_t vr_peek(const VR &r) { uint32_t p = (uint32_t)(r.c >> 32); asm("" : "+s"(p)); return p; }
DEV void vr_skip(VR &r, int k) { r.c <<= k; r.n -= k; }
DEV uint32_t vr_pos(const VR &r) { return r.wi * 32u - (uint32_t)r.n; }
DEV void vr_load_windows(VR &r, const uint32_t *ring32) {
    const int lane = threadIdx.x;
    r.w0 = (int)ring32[(r.wb + lane) & RING_WMASK];
    r.w1 = (int)ring32[(r.wb + 64 + lane) & RING_WMASK];
}
DEV void vr_seek(VR &r, const uint32_t *ring32, uint32_t pos) {
    r.wi = pos >> 5; r.wb = r.wi & ~15u; r.c = 0; r.n = 0;
    vr_load_windows(r, ring32);
    vr_fill(r); vr_fill(r);
    vr_skip(r, (int)(pos & 31));
}
// at a macroblock boundary: reload both windows 16-dword aligned once the reader is 16 dwords in; top
// the LDS ring up first when the reader is within half a ring of its write head (ring_fill overwrites
// only dwords below wb)
DEV void vr_slide(VR &r, Ring &RS, uint8_t *ring, uint32_t &refill_at) {
    if (r.wi - r.wb >= 16) {
        r.wb = r.wi & ~15u;
        if (r.wb >= refill_at) { ring_fill(RS, ring, r.wb * 4 + RING_BYTES - 128); refill_at = ring_refill_at(RS); }
        vr_load_windows(r, (const uint32_t *)ring);
    }
}
DEV void vr_reslide(VR &r, const uint8_t *ring) {
    if (__builtin_expect(r.wi - r.wb >= 40, 0)) {
        r.wb = r.wi & ~15u;
        vr_load_windows(r, (const uint32_t *)ring);
    }
}
DEV uint32_t vr_ue_long(VR &r, int lz) {  // codeNum >= 65535: rare
    if (lz >= 32) { r.err = 1; return 0; }
    vr_skip(r, lz);
    vr_fill(r);
    const uint32_t v = (uint32_t)(r.c >> (63 - lz));
    vr_skip(r, lz + 1);
    return v - 1u;
}
DEV uint32_t vr_ue(VR &r) {
    vr_fill(r);
    const uint32_t p = vr_peek(r);
    const int lz = __clz(p);
    if (__builtin_expect(lz >= 16, 0)) return vr_ue_long(r, lz);
    const int len = 2 * lz + 1;
    vr_skip(r, len);
    return (p >> (32 - len)) - 1u;
}
DEV int vr_se(VR &r) {
    const uint32_t k = vr_ue(r);
    return (k & 1) ? (int)((k + 1) >> 1) : -(int)(k >> 1);
}

// register-resident tables (vlc_tables.inc ParseTables), one VGPR per 64-entry row
struct PT { int ct[6], ctdc, tz[2], rb, cbp, qpc, q1; };
DEV void pt_load(PT &t) {
    const int lane = threadIdx.x;
    GLOBAL const uint32_t *g = (GLOBAL const uint32_t *)(uint64_t)&g_PT.v[0][0];
#pragma unroll
    for (int k = 0; k < 6; k++) t.ct[k] = (int)g[k * 64 + lane];
    t.ctdc = (int)g[6 * 64 + lane];
    t.tz[0] = (int)g[7 * 64 + lane]; t.tz[1] = (int)g[8 * 64 + lane];
    t.rb = (int)g[9 * 64 + lane]; t.cbp = (int)g[10 * 64 + lane]; t.qpc = (int)g[11 * 64 + lane]; t.q1 = (int)g[12 * 64 + lane];
}

// ---------------------------------------------------------------- 9.2 residual_block_cavlc
// nC >= 0 (chroma DC: read_cdc). Returns TotalCoeff; the level at scan index k lands in lane base+k
// of `val` (other lanes 0). Errors accumulate in r.err; decoding continues on clamped values (every
// index stays in range), so the common path has no early exits.
DEV uint32_t coeff_token(VR &r, const PT &T, int nc) {  // -> len | t1 << 5 | tc << 8, 0 = no code
    vr_fill(r);
    const uint32_t p = vr_peek(r);
    if (nc >= 8) {  // 6-bit fixed-length code
        const uint32_t v = p >> 26, tcv = (v >> 2) + 1, t1v = v & 3;
        return v == 3 ? 6u : (t1v <= min(tcv, 3u) ? (6u | t1v << 5 | tcv << 8) : 0u);
    }
    const int lz = min(__clz(p), 15);
    const uint32_t idx = (uint32_t)lz * 8 + ((p << lz << 1) >> 29);
    const int ix = (int)(idx & 63);
    uint32_t a, b;
    if (nc < 2) { a = rdlane(T.ct[0], ix); b = rdlane(T.ct[1], ix); }
    else if (nc < 4) { a = rdlane(T.ct[2], ix); b = rdlane(T.ct[3], ix); }
    else { a = rdlane(T.ct[4], ix); b = rdlane(T.ct[5], ix); }
    return idx < 64 ? a : b;
}
DEV int read_block(VR &r, const PT &T, int maxnum, int nc, int base, int &val) {
    const int lane = threadIdx.x;
    val = 0;
    if (nc < 2) {
        // the commonest coded block: coeff_token "01" (TotalCoeff 1, TrailingOnes 1), its sign, and
        // total_zeros of Table 9-7 for TotalCoeff 1: "1" -> 0, "0{k}1b" -> 2k - b (k = 1..7),
        // "00000000 1" -> 15 -- no table, no run_before
        vr_fill(r);
        const uint32_t p = vr_peek(r);
        if ((int)p < 0) { vr_skip(r, 1); return 0; }  // "1": TotalCoeff 0
        if ((p >> 30) == 1u) {
            const uint32_t q = p << 3;
            const int k = __clz(q | 0x7fu);  // leading zeros of total_zeros, capped at 24 (invalid > 8)
            if (__builtin_expect(k <= 7, 1)) {
                const int tz = k == 0 ? 0 : 2 * k - (int)((q << k << 1) >> 31);
                vr_skip(r, 3 + (k == 0 ? 1 : k + 2));
                val = wrlane((p >> 29) & 1 ? 0xffffffffu : 1u, (base + tz) & 63, 0);
                return 1;
            }
        }
    }
    const uint32_t e = coeff_token(r, T, nc);
    vr_skip(r, (int)(e & 31));
    const int tc = min((int)(e >> 8), maxnum);
    uint32_t bad = e == 0 || (int)(e >> 8) > maxnum;
    if (tc == 0) { r.err |= bad; return 0; }
    // ---- levels (9.2.2): trailing ones, then prefix/suffix codes; level i in lane i of lv
    const int t1 = (int)((e >> 5) & 3);
    const uint32_t signs = (vr_peek(r) >> 1) >> (31 - t1);  // t1 sign bits (0 when t1 == 0)
    vr_skip(r, t1);
    int lv = lane < t1 ? (((signs >> (t1 - 1 - lane)) & 1) ? -1 : 1) : 0;
    int sl = (tc > 10 && t1 < 3) ? 1 : 0;
    for (int i = t1; i < tc; i++) {
        vr_fill(r);
        const uint32_t q = vr_peek(r);
        const int prefix = min(__clz(q), 15);  // level_prefix > 15 is not Baseline
        bad |= q < 0x10000u;
        const int ssize = prefix == 15 ? 12 : ((prefix == 14 && sl == 0) ? 4 : sl);
        const uint32_t suf = ((q << prefix << 1) >> 1) >> (31 - ssize);  // ssize bits (0 when ssize == 0)
        vr_skip(r, prefix + 1 + ssize);
        int code = (prefix << sl) + (int)suf;
        if (prefix == 15 && sl == 0) code += 15;
        if (i == t1 && t1 < 3) code += 2;
        const int level = (code & 1) ? (-code - 1) >> 1 : (code + 2) >> 1;
        lv = wrlane((uint32_t)level, i, lv);
        sl = max(sl, 1);
        if (iabs(level) > ((3 << sl) >> 1) && sl < 6) sl++;  // 3 << (sl - 1) without a clamp on the vector unit
    }
    // ---- total_zeros (9.2.3)
    int tz = 0;
    if (tc < maxnum) {
        vr_fill(r);
        const uint32_t q = vr_peek(r);
        const int lz = __clz(q);
        uint32_t bi;
        if (tc == 1) { const int l8 = min(lz, 8); bi = (uint32_t)l8 * 2 + ((q << l8 << 1) >> 31); bad |= lz > 8; }
        else { const int lzc = min(lz, 6); bi = 18u + (uint32_t)(tc - 2) * 28 + (uint32_t)lzc * 4 + ((q << lzc << 1) >> 30); }
        const uint32_t dw = bi >> 2;
        const uint32_t a = rdlane(T.tz[0], (int)(dw & 63)), b = rdlane(T.tz[1], (int)(dw & 63));
        const uint32_t ent = ((dw < 64 ? a : b) >> ((bi & 3) * 8)) & 255;
        bad |= ent == 0;
        vr_skip(r, (int)(ent >> 4));
        tz = (int)(ent & 15);
    }
    // ---- run_before (9.2.4) and the scatter of level i to scan position base + pos
    int zl = tz, pos = tz + tc - 1;
    bad |= pos >= maxnum;
    for (int i = 0; i < tc - 1; i++) {
        int rb = 0;
        if (zl > 0) {
            vr_fill(r);
            const uint32_t q = vr_peek(r);
            const uint32_t ent = rdlane(T.rb, (int)((zl <= 6 ? (uint32_t)(zl - 1) * 8 : 48u) + (q >> 29)));
            if (__builtin_expect(ent != 0, 1)) { rb = (int)(ent & 15); vr_skip(r, (int)(ent >> 4)); }
            else {  // zerosLeft > 6, code 000 1.. : run_before = 4 + leading zeros
                const int lz = min(__clz(q), 10);
                bad |= q < 0x200000u;
                rb = lz + 4;
                vr_skip(r, lz + 1);
            }
        }
        val = wrlane(rdlane(lv, i), (base + pos) & 63, val);
        pos -= rb + 1;
        zl -= rb;
    }
    val = wrlane(rdlane(lv, tc - 1), (base + pos) & 63, val);
    bad |= zl < 0 || pos < 0;
    r.err |= bad;
    return tc;
}

// Chroma DC (nC = -1, maxNumCoeff 4) with the levels kept in SGPRs: returns the four coefficients in
// scan order as packed int16 (one 8-byte store) and TotalCoeff.
#ifndef H264MI_HDR_FAST
#define H264MI_HDR_FAST 1
#endif
#ifndef H264MI_CDC_FAST
#define H264MI_CDC_FAST 2
#endif
DEV int read_cdc(VR &r, const PT &T, uint64_t &packed) {
    packed = 0;
    vr_fill(r);
    const uint32_t p = vr_peek(r);
    if (H264MI_CDC_FAST) {
        // the two commonest chroma DC blocks without a table: coeff_token "1" (TotalCoeff 1, TrailingOnes
        // 1), its sign and total_zeros of Table 9-9a for TotalCoeff 1 ("1" 0, "01" 1, "001" 2, "000" 3),
        // no run_before; and "01" (TotalCoeff 0)
        if ((int)p < 0) {
            const int tz = min(__clz(p << 2), 3);
            vr_skip(r, 2 + (tz == 3 ? 3 : tz + 1));
            packed = (uint64_t)((p >> 30) & 1 ? 0xffffu : 1u) << (16 * tz);
            return 1;
        }
        if ((p >> 30) == 1u) { vr_skip(r, 2); return 0; }
        if (H264MI_CDC_FAST > 1 && (p >> 29) == 1u) {
            // "001": TotalCoeff 2, TrailingOnes 2 -- two sign bits, total_zeros of Table 9-9a for
            // TotalCoeff 2 ("1" 0, "01" 1, "00" 2), run_before of the first level for zerosLeft 1 ("1" 0,
            // "0" 1) or 2 ("1" 0, "01" 1, "00" 2); the second level takes the remaining zeros
            const uint32_t q = p << 5;
            const int tz = (int)(q >> 31) ? 0 : ((q >> 30) == 1u ? 1 : 2);
            int used = 5 + (tz == 0 ? 1 : 2);
            const uint32_t u = p << used;
            int rb = 0;
            if (tz == 1) { rb = (int)(u >> 31) ? 0 : 1; used += 1; }
            else if (tz == 2) { rb = (int)(u >> 31) ? 0 : ((u >> 30) == 1u ? 1 : 2); used += (int)(u >> 31) ? 1 : 2; }
            vr_skip(r, used);
            packed = ((uint64_t)((p >> 28) & 1 ? 0xffffu : 1u) << (16 * (tz + 1))) | ((uint64_t)((p >> 27) & 1 ? 0xffffu : 1u) << (16 * (tz - rb)));
            return 2;
        }
    }
    const int lz = min(__clz(p), 7);
    const uint32_t e = rdlane(T.ctdc, lz * 8 + (int)((p << lz << 1) >> 29));
    if (!e) { r.err = 1; return 0; }
    vr_skip(r, (int)(e & 31));
    const int tc = (int)(e >> 8), t1 = (int)((e >> 5) & 3);
    if (tc == 0) return 0;
    uint64_t lvp = 0;  // level i (decoding order) in bits 16i..16i+15
    if (t1) {
        const uint32_t signs = vr_peek(r) >> (32 - t1);
        vr_skip(r, t1);
        for (int k = 0; k < t1; k++) lvp |= (uint64_t)(((signs >> (t1 - 1 - k)) & 1) ? 0xffffu : 1u) << (16 * k);
    }
    int sl = 0;
    for (int i = t1; i < tc; i++) {
        vr_fill(r);
        const uint32_t q = vr_peek(r);
        const int prefix = __clz(q);
        if (prefix > 15) { r.err = 1; return tc; }
        const int ssize = (prefix == 14 && sl == 0) ? 4 : (prefix == 15 ? 12 : sl);
        const uint32_t suf = ssize ? ((q << prefix << 1) >> (32 - ssize)) : 0u;
        vr_skip(r, prefix + 1 + ssize);
        int code = (prefix << sl) + (int)suf;
        if (prefix == 15 && sl == 0) code += 15;
        if (i == t1 && t1 < 3) code += 2;
        const int level = (code & 1) ? (-code - 1) >> 1 : (code + 2) >> 1;
        lvp |= (uint64_t)((uint32_t)level & 0xffffu) << (16 * i);
        if (sl == 0) sl = 1;
        if (iabs(level) > ((3 << sl) >> 1) && sl < 6) sl++;
    }
    int tz = 0;
    if (tc < 4) {
        vr_fill(r);
        const uint32_t q = vr_peek(r);
        const uint32_t k = tc == 1 ? TZDC_K1 : (tc == 2 ? TZDC_K2 : TZDC_K3);
        const uint32_t nib = (k >> ((q >> 29) * 4)) & 15;
        if (!(nib >> 2)) { r.err = 1; return tc; }
        vr_skip(r, (int)(nib >> 2));
        tz = (int)(nib & 3);
    }
    int zl = tz, pos = tz + tc - 1;
    if (pos >= 4) { r.err = 1; return tc; }
    for (int i = 0; i < tc; i++) {
        int rb = 0;
        if (i < tc - 1 && zl > 0) {
            vr_fill(r);
            const uint32_t ent = rdlane(T.rb, (zl - 1) * 8 + (int)(vr_peek(r) >> 29));
            rb = (int)(ent & 15);
            vr_skip(r, (int)(ent >> 4));
        } else if (i == tc - 1) rb = zl;
        packed |= ((lvp >> (16 * i)) & 0xffffull) << (16 * pos);
        pos -= rb + 1;
        zl -= rb;
    }
    if (zl < 0 || pos < -1) r.err = 1;
    return tc;
}

// nC (9.2.1) from the neighbours' TotalCoeff, 0xff = not available
DEV int nc_of(uint32_t na, uint32_t nb) {
    const uint32_t both = (na + nb + 1) >> 1;
    uint32_t t = na == 0xffu ? nb : both;
    t = nb == 0xffu ? na : t;
    return t == 0xffu ? 0 : (int)t;
}

#ifndef H264MI_BLK_ASM
#define H264MI_BLK_ASM 1
#endif
#ifndef H264MI_P_ASM
#define H264MI_P_ASM 1  // P-slice macroblock run in one asm statement (cavlc_blk.inc p_mb_run)
#endif
#ifndef H264MI_I_ASM
#define H264MI_I_ASM 1  // I slices through the same asm macroblock run (no mb_skip_run; I_NxN and I_16x16 in asm)
#endif
#include "cavlc_blk.inc"

// ---------------------------------------------------------------- SPS / PPS (7.3.2.1, 7.3.2.2)
// ps lives in LDS; lane 0 writes it (only on success), the barrier publishes it to the wave.
DEV bool parse_sps(Bits &b, DecParams &ps, int mbw_alloc, int mbh_alloc) {
    const int profile = br_bits(b, 8);
    br_bits(b, 16);
    br_ue(b);
    if (profile == 100 || profile == 110 || profile == 122 || profile == 244 || profile == 44 || profile == 83 ||
        profile == 86 || profile == 118 || profile == 128) return false;
    const int log2_mfn = br_ue(b) + 4;
    const int poc_type = br_ue(b);
    int log2_poc = 0, dpoaz = 0;
    if (poc_type == 0) log2_poc = br_ue(b) + 4;
    else if (poc_type == 1) {
        dpoaz = (int)br_bits(b, 1); br_se(b); br_se(b);
        const uint32_t n = br_ue(b);
        if (n > 255) return false;
        for (uint32_t i = 0; i < n; i++) br_se(b);
    }
    br_ue(b); br_bits(b, 1);
    const int mbw = br_ue(b) + 1, mbh = br_ue(b) + 1;
    if (!br_bits(b, 1)) return false;  // frame_mbs_only_flag
    br_bits(b, 1);
    int crop[4] = {0, 0, 0, 0};
    if (br_bits(b, 1)) for (int i = 0; i < 4; i++) crop[i] = br_ue(b);
    if (b.err || mbw != mbw_alloc || mbh != mbh_alloc || log2_mfn > 16 || log2_poc > 16) return false;
    __syncthreads();
    if (threadIdx.x == 0) {
        ps.have_sps = 1; ps.mbw = mbw; ps.mbh = mbh; ps.log2_mfn = log2_mfn; ps.poc_type = poc_type; ps.log2_poc = log2_poc;
        ps.dpoaz = dpoaz;
        for (int i = 0; i < 4; i++) ps.crop[i] = crop[i];
    }
    __syncthreads();
    return true;
}
DEV bool parse_pps(Bits &b, DecParams &ps) {
    br_ue(b); br_ue(b);
    if (br_bits(b, 1)) return false;  // CABAC: not Baseline
    const int bfp = br_bits(b, 1);
    if (br_ue(b) != 0) return false;  // FMO
    const int nref = br_ue(b) + 1;
    br_ue(b);
    const int weighted = br_bits(b, 1);
    br_bits(b, 2);
    const int qp = 26 + br_se(b);
    br_se(b);
    const int cqp = br_se(b);
    const int dbkc = br_bits(b, 1), cip = br_bits(b, 1), red = br_bits(b, 1);
    if (b.err || cip || weighted || cqp < -12 || cqp > 12) return false;
    __syncthreads();
    if (threadIdx.x == 0) { ps.have_pps = 1; ps.bfp = bfp; ps.nref = nref; ps.qp = qp; ps.cqp = cqp; ps.dbkc = dbkc; ps.red = red; }
    __syncthreads();
    return true;
}

// ---------------------------------------------------------------- NAL scan kernel
// One wave per (frame slot, stream): start codes, NAL types, emulation-prevention count and the
// rbsp_stop_one_bit position of every NAL the decoder consumes, into the slot's DecFrame.
struct DecScanLaunch { int S, n; const DecInput *in; const DecDesc *desc; };  // desc: first slot of the call
// Both passes read the access unit SCAN_CHUNKS x 64 bytes at a time, one byte per lane per chunk,
// with every load of a batch issued before the first use (one memory wait per batch, not per 64 B:
// the scan sits on the latency path of every decode call). Neighbour bytes come from lane shuffles
// across chunk boundaries instead of extra loads.
constexpr int SCAN_CHUNKS = 8;
DEV void scan_load(GLOBAL const uint8_t *in, int base, int end, int fill, int (&b)[SCAN_CHUNKS + 1]) {
#pragma unroll
    for (int k = 0; k <= SCAN_CHUNKS; k++) {
        const int i = base + 64 * k + (int)threadIdx.x;
        const int v = in[min(i, end - 1)];  // unconditional (see ring_fill); callers: end > base
        b[k] = i < end ? v : fill;
    }
}
__global__ __launch_bounds__(64) void dec_scan_kernel(DecScanLaunch a) {
    __shared__ int s_nal[H264MI_MAX_NALS];
    __shared__ int s_nnal;
    const int lane = threadIdx.x, w = blockIdx.x;
    if (w >= a.S * a.n) return;
    const DecInput *I = a.in + w;
    GLOBAL DecFrame *F = uni_ptr(a.desc[w].frm);
    const uint8_t *in_generic = I->nal;
    GLOBAL const uint8_t *in = uni_ptr(in_generic);
    const int32_t *szp = I->size_dev;
    const int nbytes = uni(szp ? *szp : I->size);
    int nfound = 0;  // wave-uniform
    if (in_generic && nbytes > 0) {
        // pass 1: start codes 00 00 01 (NAL header byte at p + 3), in stream order
        for (int c0 = 0; c0 < nbytes && nfound < H264MI_MAX_NALS; c0 += 64 * SCAN_CHUNKS) {
            int b[SCAN_CHUNKS + 1];
            scan_load(in, c0, nbytes, 0xff, b);
#pragma unroll
            for (int k = 0; k < SCAN_CHUNKS; k++) {
                const int i = c0 + 64 * k + lane;
                // bytes i + 1, i + 2 (all shuffles unconditional, then selected per lane)
                const int x1 = __shfl(b[k], (lane + 1) & 63), x2 = __shfl(b[k], (lane + 2) & 63);
                const int h0 = (int)rdlane(b[k + 1], 0), h1 = (int)rdlane(b[k + 1], 1);
                const int n1 = lane < 63 ? x1 : h0;
                const int n2 = lane < 62 ? x2 : (lane == 62 ? h0 : h1);
                uint64_t m = __ballot(i + 2 < nbytes && b[k] == 0 && n1 == 0 && n2 == 1);
                while (m && nfound < H264MI_MAX_NALS) {
                    const int bpos = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (lane == 0) s_nal[nfound] = c0 + 64 * k + bpos + 3;
                    nfound++;
                }
            }
        }
    }
    if (lane == 0) s_nnal = nfound;
    __syncthreads();
    const int nn = uni(s_nnal);
    int cnt = 0, nsl = 0, err = 0;
    for (int k = 0; k < nn; k++) {
        const int s = uni(s_nal[k]);
        int e = k + 1 < nn ? uni(s_nal[k + 1]) - 3 : nbytes;
        while (e > s && uni((uint32_t)in[e - 1]) == 0) e--;
        if (e - s < 1) continue;
        const int type = uni((uint32_t)in[s]) & 31;
        if (type != 1 && type != 5 && type != 7 && type != 8) continue;
        // pass 2 over the payload [s + 1, e): emulation-prevention bytes (03 after 00 00, not before
        // payload byte 2) and the last byte that is neither zero nor removed (it holds the stop bit).
        // c1 / c2: the two bytes before the current chunk (0xff before the payload: no match)
        uint32_t removed_total = 0;
        int last_nz = -1, last_rm_before = 0, c1 = 0xff, c2 = 0xff;
        for (int c0 = s + 1; c0 < e; c0 += 64 * SCAN_CHUNKS) {
            int b[SCAN_CHUNKS + 1];
            scan_load(in, c0, e, 0, b);
#pragma unroll
            for (int q = 0; q < SCAN_CHUNKS; q++) {
                if (c0 + 64 * q >= e) break;
                const int i = c0 + 64 * q + lane;
                const bool valid = i < e;
                const int bv = b[q];
                int p1 = __shfl(bv, (lane + 63) & 63), p2 = __shfl(bv, (lane + 62) & 63);
                if (lane == 0) { p1 = c1; p2 = c2; }
                if (lane == 1) p2 = c1;
                const bool rm = valid && bv == 3 && p1 == 0 && p2 == 0;
                const uint64_t mr = __ballot(rm);
                const uint64_t mn = __ballot(valid && bv != 0 && !rm);
                if (mn) {
                    const int hi = 63 - __clzll((long long)mn);
                    last_nz = c0 + 64 * q + hi;
                    const uint64_t below = hi == 63 ? mr : (mr & ((2ull << hi) - 1));
                    last_rm_before = (int)removed_total + __popcll(below);
                }
                removed_total += (uint32_t)__popcll(mr);
                c2 = (int)rdlane(bv, 62); c1 = (int)rdlane(bv, 63);
            }
        }
        if (last_nz < 0) continue;
        const uint32_t rb_idx = (uint32_t)(last_nz - (s + 1) - last_rm_before);
        const int lb = uni((uint32_t)in[last_nz]);
        const uint32_t stop = rb_idx * 8 + (7 - (__ffs(lb) - 1));
        if (type == 1 || type == 5) {  // a slice of the picture (any number, any order)
            if (nsl >= H264MI_MAX_SLICES) err = 2;
            else { if (lane == 0) F->sl[nsl].nal = cnt; nsl++; }
        }
        if (lane == 0) { F->e[cnt].start = s; F->e[cnt].end = e; F->e[cnt].type = type; F->e[cnt].stop = stop; }
        cnt++;
    }
    if (lane == 0) {
        F->nal = in_generic; F->nbytes = nbytes; F->nnal = cnt; F->nsl = nsl; F->err = err;
        F->got_pic = 0; F->nonref = 0; F->anyp = 0;
    }
}

// ---------------------------------------------------------------- slice parse
DEV void open_nal(Ring &RS, uint8_t *ring, GLOBAL const uint8_t *in, int s, int e, Bits &b, uint32_t &refill_at,
                  uint32_t fill = RING_BYTES - 128) {
    __syncthreads();
    if (threadIdx.x == 0) { RS.in = in; RS.in_pos = s + 1; RS.in_end = e; RS.c1 = 0xff; RS.c2 = 0xff; RS.written = 0; }
    __syncthreads();
    ring_fill(RS, ring, fill);
    refill_at = ring_refill_at(RS);
    b.ring32 = (const uint32_t *)ring; b.cache = 0; b.avail = 0; b.widx = 0; b.err = 0;
}

// Contexts of the coeff_token tables (9.2.1) ride in SGPRs: L holds, per 4x4 row of the macroblock,
// the TotalCoeff of the block decoded last in that row (on entry: the left macroblock's right column),
// T the same per column (on entry: the bottom row of the macroblock above, read from LDS), and LC / TC
// the chroma AC equivalents (bytes Cb0, Cb1, Cr0, Cr1). In decoding order the block decoded last in a
// row / column is exactly the left / upper neighbour, so nA / nB are byte extracts. 0xff = not
// available (picture edge). After the macroblock L / LC are the next one's left context and T / TC go
// to LDS for the macroblock below.
// 7.3.3 slice_header() -> SliceHdr (the slice-data pass starts at data_pos). info: the slice word every
// record of the slice carries (h264mi_types.h MB_SLICE_*)
struct SliceHdr { int ok, slt, qp, first_mb; uint32_t info, data_pos; };
DEV SliceHdr parse_slice_header(Bits &b, int nal_type, int nal_ref_idc, const DecParams &ps, int total) {
    SliceHdr out = {0, 0, 0, 0, 0, 0};
    if (!uni(ps.have_sps) || !uni(ps.have_pps)) return out;
    if (nal_type == 5 && nal_ref_idc == 0) return out;  // an IDR picture is a reference picture
    const uint32_t first_mb = br_ue(b);
    const int slt = (int)(br_ue(b) % 5);
    br_ue(b);
    if (first_mb >= (uint32_t)total || (slt != 0 && slt != 2) || (nal_type == 5 && slt != 2)) return out;
    br_bits(b, uni(ps.log2_mfn));
    if (nal_type == 5) br_ue(b);
    const int poc_type = uni(ps.poc_type), bfp = uni(ps.bfp);
    if (poc_type == 0) { br_bits(b, uni(ps.log2_poc)); if (bfp) br_se(b); }
    else if (poc_type == 1 && !uni(ps.dpoaz)) { br_se(b); if (bfp) br_se(b); }
    if (uni(ps.red)) br_ue(b);
    int nref = uni(ps.nref);
    if (slt == 0) {
        if (br_bits(b, 1)) nref = br_ue(b) + 1;
        if (br_bits(b, 1)) { for (int g = 0; g < 64; g++) { uint32_t op = br_ue(b); if (op == 3 || b.err) break; br_ue(b); } }
        if (nref > 1) return out;  // (a P slice without an earlier picture is rejected at reconstruction)
    }
    if (nal_ref_idc == 0) {
        // a non-reference picture: no dec_ref_pic_marking() (7.3.3); decoded and output, the reference stays
    } else if (nal_type == 5) br_bits(b, 2);
    else if (br_bits(b, 1)) {
        for (int g = 0; g < 64; g++) {
            uint32_t op = br_ue(b);
            if (op == 0 || b.err) break;
            if (op == 1 || op == 3) br_ue(b);
            if (op == 2) br_ue(b);
            if (op == 3 || op == 6) br_ue(b);
            if (op == 4) br_ue(b);
        }
    }
    const int qp = uni(ps.qp) + br_se(b);
    // loop-filter parameters of the slice: disable_deblocking_filter_idc (0 filter, 1 off, 2 not across
    // slice edges) and slice_alpha_c0 / beta offset_div2, packed into the slice word
    uint32_t idc = 0, fa = 0, fb = 0;
    if (uni(ps.dbkc)) {
        idc = br_ue(b);
        if (idc > 2) return out;
        if (idc != 1) {
            const int a = br_se(b), c = br_se(b);
            if (a < -6 || a > 6 || c < -6 || c > 6) return out;
            fa = (uint32_t)a & 15u; fb = (uint32_t)c & 15u;
        }
    }
    if (b.err || qp < 0 || qp > 51) return out;
    out.ok = 1; out.slt = slt; out.qp = qp; out.first_mb = (int)first_mb; out.data_pos = br_pos(b);
    out.info = first_mb | (idc << 20) | (fa << 22) | (fb << 26);
    return out;
}

#ifndef H264MI_SLT_TEMPLATE
#define H264MI_SLT_TEMPLATE 1
#endif
// SLT: the slice type as a compile-time constant (0 P, 2 I; -1 = read from `slt`): one specialised MB
// loop per slice type, so no slice-type test is left on the chain
// One slice: macroblocks first_mb .. end_mb - 1 (end_mb out). Its neighbours in other slices are not
// available: the row-above contexts start as "not available" and only this slice's macroblocks write
// them; the left context starts "not available". sinfo rides in every record (dword 31, MB_SLICE_*).
// Streamed reconstruction (DESIGN.md §6): the records of MB rows 0..k-1 are handed to dec_recon_kernel
// while the slice is still being parsed. At a row end: wait for every store issued so far (and for the
// L2 write-back issued at the previous row end), publish the rows that write-back covered with an
// agent-scope store of {tag, rows}, and issue the next write-back (buffer_wbl2 sc1: this XCD's dirty L2
// lines to memory) without waiting for it -- the next row end waits, by which time it is long done.
DEV void pub_rows(GLOBAL uint64_t *prog, uint32_t tag, int &pending, int rows) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (pending > 0 && threadIdx.x == 0)
        __hip_atomic_store(prog, ((uint64_t)tag << 32) | (uint32_t)pending, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("buffer_wbl2 sc1" ::: "memory");
    pending = rows;
}
#ifdef H264MI_ASM_CNT
__device__ uint64_t g_asm_cnt[16];
extern "C" int h264mi_debug_asm_counts(uint64_t *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_asm_cnt), sizeof(g_asm_cnt)) != hipSuccess) return -1;
    if (reset) { static const uint64_t z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_asm_cnt), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
template <bool PROF, int SLT>
DEV bool parse_slice_data(Ring &RS, uint8_t *ring, uint32_t *rows, uint32_t refill_at, uint32_t stop, int slt_rt, int qp,
                          int cqp, uint32_t data_pos, int mbw, int mbh, GLOBAL uint32_t *g_info, GLOBAL MbCoef *g_coef,
                          const PT &T, uint64_t *s_prof, uint64_t &t_prev, int first_mb, uint32_t sinfo, int &end_mb,
                          GLOBAL uint64_t *prog, uint32_t tag, int pub) {
    const int lane = threadIdx.x;
    const int slt = SLT >= 0 ? SLT : slt_rt;
    // section timer: 3 ring fill, 4 skip runs, 5 MB header, 6 residual (8 of it: mb_qp_delta + contexts,
    // 9 luma, 10 chroma DC, 11 chroma AC), 7 record
    // accumulators in (uniform) registers, written to LDS once at the end: a timer read costs the chain
    // one s_memtime + wait, not an LDS read-modify-write
    uint64_t acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0;
    auto lap = [&](int k) { if constexpr (PROF) { uint64_t t = clock64(); acc[k] += t - t_prev; t_prev = t; } };
    // event counters (PROF): 12 generic AC blocks, 13 planes skipped whole, 14 AC blocks skipped singly, 15 sum of AC TotalCoeff
    auto cnt = [&](int k, int v) { if constexpr (PROF) acc[k] += (uint64_t)v; };
    int qpc = (int)rdlane(T.qpc, clip3(0, 51, qp + cqp));
    // ---- 4. slice_data(): symbols only. Motion vectors and Intra4x4 modes are NOT derived here:
    // the record carries mvd (at each partition's first 4x4 block) and the raw intra mode codes,
    // and dec_recon_kernel resolves them in its MB-row wavefront (their predictions need only
    // the neighbours the wavefront already has). What stays on the serial chain is what the
    // bitstream syntax itself depends on: nnz contexts (coeff_token tables) and QP.
    const uint32_t *ring32 = (const uint32_t *)ring;
    VR r;
    r.err = 0;
    vr_seek(r, ring32, data_pos);
    for (int i = lane; i < 2 * mbw; i += 64) rows[i] = 0xffffffffu;  // row above the picture: not available
    __syncthreads();
    const int total = mbw * mbh;
    const int rec_init = lane >= 2 && lane <= 5 ? 0x02020202 : (lane == 31 ? (int)sinfo : 0);  // i4mode bytes 2 (DC) of non-I4 records; the slice word
    const uint32_t off2 = 2u * (uint32_t)lane, off4 = 4u * (uint32_t)lane;  // per-lane byte offsets of the masked stores
    int addr = first_mb, cx = first_mb % mbw;
    int pub_pending = 0, pub_next = mbw;  // streamed reconstruction: rows written back, next row end
    int asm_cnt = 0;  // H264MI_ASM_CNT builds: event counts of the asm MB run (lane = event)
    bool more = true, fail = false;
    uint32_t L = 0xffffffffu, LC = 0xffffffffu;  // left contexts (0xff: picture edge)
    // p_mb_run (cavlc_blk.inc): block k's ys | xs << 8 | slot << 16 (luma 0..15 in decoding order, chroma AC 16..23)
    int vdesc = 0;
    {
        const int k = lane & 31;
        int ys, xs, sl;
        if (k < 16) { ys = ((k & 8) << 1) | ((k & 2) << 2); xs = ((k & 4) << 2) | ((k & 1) << 3); sl = (ys >> 1) + (xs >> 3); }
        else { const int o = k - 16, pl = o >> 2, bk = o & 3; ys = 16 * pl + 8 * (bk >> 1); xs = 16 * pl + 8 * (bk & 1); sl = k; }
        vdesc = ys | xs << 8 | sl << 16;
    }
    // p_mb_run's quiet luma quarter: lane -> byte offset of its block (lane >> 4, decoding order) from the
    // quarter's first block in MbCoef::luma (raster slots base, base + 1, base + 4, base + 5), and the byte of
    // the quarter's TotalCoeff word for the lane's vnz slot
    const int vlq = 2 * (lane & 15) + 32 * ((lane >> 4) & 1) + 128 * (lane >> 5);
    const int vsh8l = 8 * (((lane >> 2) & 1) * 2 + (lane & 1));
    const uint32_t rows_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint32_t *)rows;
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint8_t *)ring;
    while (more && addr < total && !fail) {
        if (pub && addr >= pub_next) {  // a row end: hand the finished rows to the reconstruction
            const int rdone = addr / mbw;
            pub_rows(prog, tag, pub_pending, rdone);
            pub_next = (rdone + 1) * mbw;
        }
        vr_slide(r, RS, ring, refill_at);
        uint32_t pre_mt = ~0u;  // mb_type already read by p_mb_run
        if constexpr ((SLT == 0 || (SLT == 2 && H264MI_I_ASM)) && H264MI_P_ASM) {
            uint32_t mtv = 0;
            const int ex = p_mb_run(r, T, L, LC, qp, qpc, cqp, addr, cx, mbw, total, stop, refill_at, g_info, g_coef, rows_lds,
                                    ring_lds, vdesc, rec_init, mtv, pub, asm_cnt, vlq, vsh8l, SLT == 2 ? 4 : 0);
            if (ex == 0) break;
            if (ex == 1) { fail = true; break; }
            if (ex == 2) continue;  // vr_slide tops the ring up
            if (ex == 4) {          // a row end (streamed reconstruction): the row-end checks, then publish
                if (addr >= total || vr_pos(r) >= stop) break;
                continue;
            }
            pre_mt = mtv;
        }
        bool mt0 = false;  // P slice, bits "11": mb_skip_run 0 and mb_type 0 (P_L0_16x16) read at once
        if (slt == 0 && H264MI_HDR_FAST && pre_mt == ~0u) {
            vr_fill(r);
            if ((vr_peek(r) >> 30) == 3u) { vr_skip(r, 2); mt0 = true; }
        }
        if (slt == 0 && !mt0 && pre_mt == ~0u) {
            const uint32_t run = vr_ue(r);
            if (r.err || run > (uint32_t)(total - addr)) { fail = true; break; }
            if (run) {  // P_Skip records: type, QP; motion derived in reconstruction (8.4.1.1)
                int rec = wrlane(MI_PSKIP | ((uint32_t)qp << 8), 0, rec_init);
                rec = wrlane((uint32_t)qpc << 8, 1, rec);
                for (uint32_t i = 0; i < run; i++) {
                    st_u32_l32(g_info + (size_t)addr * 32, off4, rec);
                    if (lane < 2) rows[2 * cx + lane] = 0u;
                    addr++;
                    if (++cx == mbw) cx = 0;
                }
                L = cx == 0 ? 0xffffffffu : 0u;
                LC = L;
                more = vr_pos(r) < stop;
            }
            lap(4);
            if (!more || addr >= total) break;
        }
        const int mbx = cx;
        // the row above's contexts for this column, read ahead of their use (LDS latency off the chain)
        const u32x2 tpre = *(const u32x2 *)&rows[2 * mbx];
        int rec = rec_init;
        int mtype, cbp = 0, i16mode = 0, cmode = 0;
        int qp_done = 0;  // mb_qp_delta already read (p16_header)
        uint32_t refd = 0xffffffffu, subs = 0;
        const uint32_t mt = pre_mt != ~0u ? pre_mt : (mt0 ? 0u : vr_ue(r));
        int itype = -1;
        if (slt == 0) { if (mt >= 5) itype = (int)mt - 5; } else itype = (int)mt;
        if (itype > 25 || (slt == 0 && mt > 30)) { fail = true; break; }
        bool ipcm = false;
        if (itype == 25) {  // I_PCM: byte-aligned raw samples
            mtype = MI_IPCM;
            ipcm = true;
            const uint32_t p0 = (vr_pos(r) + 7) & ~7u;
            const uint32_t byte0 = p0 >> 3;
            // the ring must hold the 384 samples: top it up if the reader is past the refill mark
            if ((byte0 >> 2) >= refill_at) { ring_fill(RS, ring, byte0 + RING_BYTES - 128); refill_at = ring_refill_at(RS); }
            for (int q = lane; q < 384; q += 64) ((GLOBAL uint8_t *)&g_coef[addr])[q] = ring[((byte0 + q) ^ 3) & (RING_BYTES - 1)];
            vr_seek(r, ring32, p0 + 384 * 8);
        } else if (itype >= 0) {
            if (itype == 0) {
                mtype = MI_I4;
                // raw codes in 4x4 decoding order: 0xff = prev_intra4x4_pred_mode_flag, else rem
#pragma clang loop unroll(disable)
                for (int q4 = 0; q4 < 4; q4++) {
                    uint32_t w = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        vr_fill(r);
                        const uint32_t p = vr_peek(r);
                        uint32_t code;
                        if (p >> 31) { code = 0xff; vr_skip(r, 1); }
                        else { code = (p >> 28) & 7; vr_skip(r, 4); }
                        w |= code << (8 * k);
                    }
                    rec = wrlane(w, 2 + q4, rec);
                }
                cmode = (int)vr_ue(r);
                const uint32_t cc = vr_ue(r);
                if (cc > 47) { fail = true; break; }
                cbp = (int)(rdlane(T.cbp, (int)cc) >> 8);
            } else {
                mtype = MI_I16;
                i16mode = (itype - 1) & 3;
                const int grp = (itype - 1) >> 2;  // 0..5
                cbp = ((grp >= 3 ? grp - 3 : grp) << 4) | (itype >= 13 ? 15 : 0);
                cmode = (int)vr_ue(r);
            }
            if (cmode > 3) { fail = true; break; }
        } else {
            // P macroblock (7.3.5.1 mb_pred / 7.3.5.2 sub_mb_pred), one reference: mvd of each
            // partition goes to the record slot of its first 4x4 block (raster index)
            refd = 0;
            if (H264MI_BLK_ASM && mt == 0) {  // P_L0_16x16: mvd, cbp and mb_qp_delta in one asm pass (cavlc_blk.inc)
                mtype = MI_P16x16;
                cbp = p16_header(r, T, rec, qp, qpc, cqp);
                qp_done = 1;
            } else if (mt <= 2) {
                mtype = mt == 0 ? MI_P16x16 : (mt == 1 ? MI_P16x8 : MI_P8x16);
                const int n = mt == 0 ? 1 : 2;
#if H264MI_LUMA_UNROLL || !defined(H264MI_LUMA_UNROLL)
#pragma unroll
#else
#pragma clang loop unroll(disable)
#endif
                for (int i = 0; i < n; i++) {
                    const int dx = vr_se(r), dy = vr_se(r);
                    const int ras = i == 0 ? 0 : (mt == 1 ? 8 : 2);
                    rec = wrlane(((uint32_t)dx & 0xffff) | ((uint32_t)dy << 16), 15 + ras, rec);
                }
            } else {
                mtype = MI_P8x8;
#pragma clang loop unroll(disable)
                for (int i = 0; i < 4; i++) {
                    const uint32_t sb = vr_ue(r);
                    if (sb > 3) fail = true;
                    subs |= (sb & 255) << (8 * i);
                }
                if (fail) break;
#pragma clang loop unroll(disable)
                for (int i = 0; i < 4; i++) {
                    const int sb = (subs >> (8 * i)) & 255;
                    const int np = sb == 0 ? 1 : (sb == 3 ? 4 : 2);
                    const int r0 = (i >> 1) * 8 + (i & 1) * 2;  // raster 4x4 index of the 8x8's corner
#pragma clang loop unroll(disable)
                    for (int j = 0; j < np; j++) {
                        const int dx = vr_se(r), dy = vr_se(r);
                        // sub-partition j's first 4x4: 8x4 -> rows, 4x8 -> columns, 4x4 -> raster
                        const int ras = r0 + (sb == 1 ? j * 4 : (sb == 2 ? j : (j >> 1) * 4 + (j & 1)));
                        rec = wrlane(((uint32_t)dx & 0xffff) | ((uint32_t)dy << 16), 15 + ras, rec);
                    }
                }
            }
            if (!qp_done) {
                const uint32_t cc = vr_ue(r);
                if (cc > 47) { fail = true; break; }
                cbp = (int)(rdlane(T.cbp, (int)cc) & 255);
            }
        }
        lap(5);
        int mbqp = qp, mbqpc = qpc;
        uint32_t Tl, Tc;
        uint64_t nzl = 0, nzl2 = 0, nzc = 0;  // TotalCoeff bytes for the record: luma raster 0..7, 8..15, chroma
        if (ipcm) {
            mbqpc = (int)rdlane(T.qpc, clip3(0, 51, cqp));
            L = LC = Tl = Tc = 0x10101010u;
            nzl = nzl2 = nzc = 0x1010101010101010ull;
        } else {
            if (!qp_done && (cbp || mtype == MI_I16)) {
                const int dq = vr_se(r);
                if (dq < -26 || dq > 25) { fail = true; break; }
                qp += dq;
                if (qp < 0) qp += 52; else if (qp > 51) qp -= 52;
                qpc = (int)rdlane(T.qpc, clip3(0, 51, qp + cqp));
            }
            mbqp = qp; mbqpc = qpc;
            Tl = uni(tpre.x); Tc = uni(tpre.y);
            lap(8);
            // residual() 7.3.5.3: only blocks with TotalCoeff > 0 are stored (MbCoef contract)
            GLOBAL MbCoef *cf = g_coef + addr;
            int val;
            if (mtype == MI_I16) {  // Intra16x16DCLevel: nC of block 0, the contexts are the AC blocks' (copies)
                vr_reslide(r, ring);
                if (H264MI_BLK_ASM) {
                    uint32_t Ld = L, Td = Tl;
                    uint64_t nzd = 0;
                    // the DC block is always stored (dec_recon reads it for every I16 MB): zeros when empty
                    if (!blk_decode(r, T, Ld, Td, 0, 0, 16, 0, cf->lumadc, off2, nzd, 0)) st_i16_l16(cf->lumadc, off2, 0);
                } else {
                    read_block(r, T, 16, nc_of(L & 255, Tl & 255), 0, val);
                    st_i16_l16(cf->lumadc, off2, val);
                }
            }
            const int ac = mtype == MI_I16;
            const int cbpl = ac ? ((cbp & 15) ? 15 : 0) : (cbp & 15);
            if (cbpl) {
                // blocks in decoding order; the record's TotalCoeff bytes in raster order (nzl: rows 0-1,
                // nzl2: rows 2-3, i.e. the 8x8 quarters 0-1 and 2-3)
                auto luma_half = [&](const int h, uint64_t &nz) {
#pragma clang loop unroll(disable)
                    for (int q = 0; q < 2; q++) {
                        const int i8 = 2 * h + q;
                        const uint32_t rs = (uint32_t)h * 16, cs = (uint32_t)q * 16;
                        if (!((cbpl >> i8) & 1)) { L &= ~(0xffffu << rs); Tl &= ~(0xffffu << cs); continue; }
                        vr_reslide(r, ring);
#pragma clang loop unroll(disable)
                        for (int i4 = 0; i4 < 4; i4++) {
                            const uint32_t ys = rs + (i4 >> 1) * 8, xs = cs + (i4 & 1) * 8;  // 8*y4, 8*x4
                            const uint32_t ras = (ys >> 1) + (xs >> 3);                     // y4*4 + x4
                            if (H264MI_BLK_ASM) {
                                blk_decode(r, T, L, Tl, ys, xs, 16 - ac, ac, cf->luma[ras], off2, nz, 8 * (ras - 8 * h));
                            } else {
                                const int tc = read_block(r, T, 16 - ac, nc_of((L >> ys) & 255, (Tl >> xs) & 255), ac, val);
                                L = (L & ~(255u << ys)) | ((uint32_t)tc << ys);
                                Tl = (Tl & ~(255u << xs)) | ((uint32_t)tc << xs);
                                nz |= (uint64_t)tc << (8 * (ras - 8 * h));
                                if (tc) st_i16_l16(cf->luma[ras], off2, val);
                            }
                        }
                    }
                };
                luma_half(0, nzl);
                luma_half(1, nzl2);
            } else { L = 0; Tl = 0; }
            lap(9);
            const int cbpc = cbp >> 4;
            if (cbpc) {
                uint64_t d0, d1;
                vr_reslide(r, ring);
                read_cdc(r, T, d0);
                read_cdc(r, T, d1);
                if (lane < 2) *(GLOBAL uint64_t *)&cf->cdc[lane][0] = lane ? d1 : d0;
            }
            lap(10);
            if (cbpc == 2) {
                // An AC block whose nC < 2 and whose next bit is 1 is empty (coeff_token "1"). A plane is
                // skipped in one step when its next four bits are 1111 and, with its own blocks empty,
                // every nC is < 2: nC(b0) = (l0 + t0 + 1) >> 1, nC(b1) = (t1 + 1) >> 1, nC(b2) =
                // (l1 + 1) >> 1, nC(b3) = 0 (0xff neighbours -- picture edges -- take the general path).
#pragma clang loop unroll(disable)
                for (int pl = 0; pl < 2; pl++) {
                    const uint32_t sh = 16 * pl;
                    const uint32_t l0 = (LC >> sh) & 255, l1 = (LC >> (sh + 8)) & 255;
                    const uint32_t t0 = (Tc >> sh) & 255, t1 = (Tc >> (sh + 8)) & 255;
                    vr_fill(r);
                    if ((vr_peek(r) >> 28) == 15u && l0 + t0 <= 2 && l1 <= 2 && t1 <= 2) {
                        vr_skip(r, 4);
                        LC &= ~(0xffffu << sh); Tc &= ~(0xffffu << sh);
                        cnt(13, 1);
                        continue;
                    }
                    vr_reslide(r, ring);
                    int bk0 = 0;
                    if (H264MI_BLK_ASM) {  // the plane's quiet blocks in one branch-light pass (cavlc_blk.inc)
                        uint32_t nzw = 0;
                        bk0 = cac_plane_quiet(r, LC, Tc, sh, cf->cac[pl], off2, nzw);
                        nzc |= (uint64_t)nzw << (32 * pl);
                    }
#pragma clang loop unroll(disable)
                    for (int bk = bk0; bk < 4; bk++) {
                        const int o = pl * 4 + bk;
                        const uint32_t ys = sh + 8 * (bk >> 1), xs = sh + 8 * (bk & 1);
                        if (H264MI_BLK_ASM) {
                            blk_decode(r, T, LC, Tc, ys, xs, 15, 1, cf->cac[pl][bk], off2, nzc, 8 * o);
                            continue;
                        }
                        const int nc = nc_of((LC >> ys) & 255, (Tc >> xs) & 255);
                        vr_fill(r);
                        int tc = 0;
                        if (nc < 2 && (int)vr_peek(r) < 0) { vr_skip(r, 1); cnt(14, 1); }
                        else {
                            tc = read_block(r, T, 15, nc, 1, val);
                            cnt(12, 1); cnt(15, tc);
                            nzc |= (uint64_t)tc << (8 * o);
                            if (tc) st_i16_l16(cf->cac[pl][bk], off2, val);
                        }
                        LC = (LC & ~(255u << ys)) | ((uint32_t)tc << ys);
                        Tc = (Tc & ~(255u << xs)) | ((uint32_t)tc << xs);
                    }
                }
            } else { LC = 0; Tc = 0; }
            lap(11);
        }
        lap(6);
        if (r.err || vr_pos(r) > stop) { fail = true; break; }
        // ---- the record (lane w = MbInfo dword w); mvd lanes were filled above
        rec = wrlane((uint32_t)mtype | ((uint32_t)mbqp << 8) | ((uint32_t)cbp << 16) | ((uint32_t)i16mode << 24), 0, rec);
        rec = wrlane((uint32_t)cmode | ((uint32_t)mbqpc << 8), 1, rec);
        rec = wrlane(refd, 6, rec);
        if (nzl | nzl2) {
            rec = wrlane((uint32_t)nzl, 7, rec); rec = wrlane((uint32_t)(nzl >> 32), 8, rec);
            rec = wrlane((uint32_t)nzl2, 9, rec); rec = wrlane((uint32_t)(nzl2 >> 32), 10, rec);
        }
        if (nzc) { rec = wrlane((uint32_t)nzc, 11, rec); rec = wrlane((uint32_t)(nzc >> 32), 12, rec); }
        rec = wrlane(subs, 14, rec);
        st_u32_l32(g_info + (size_t)addr * 32, off4, rec);
        if (lane < 2) rows[2 * mbx + lane] = lane ? Tc : Tl;
        addr++;
        if (++cx == mbw) { cx = 0; L = 0xffffffffu; LC = 0xffffffffu; }
        more = vr_pos(r) < stop;
        lap(7);
    }
    if constexpr (PROF) {
        if (lane == 0)
            for (int k = 3; k < 16; k++) s_prof[k] += acc[k];
    }
#ifdef H264MI_ASM_CNT
    if (lane < 16) atomicAdd((unsigned long long *)&g_asm_cnt[lane], (unsigned long long)asm_cnt);
#endif
    (void)asm_cnt;
    end_mb = addr;
    // the slice data ends exactly at the stop bit (more_rbsp_data() false), at or before the picture's end
    return !fail && !r.err && vr_pos(r) >= stop;
}

// ---------------------------------------------------------------- header kernel
// One wave per (frame slot, stream), after dec_scan_kernel: parameter sets and the slice header. The
// parameter sets in effect for frame f are those of the decoder state at the start of the call plus
// every SPS/PPS of frames 0..f-1 (and of frame f before its slice), so each wave replays them (a few
// dozen bytes) instead of waiting for the others; the last frame's wave commits them for the next
// call. Kept out of the slice-data kernel so that the MB loop has the whole register file.
// K: slice waves per (frame slot, stream) of the slice-data launch (dec_parse_kernel's grid is S * n * K;
// wave j of a frame parses its slices j, j + K, ...); the header launch ignores it.
// tag / streamed: the call's tag and whether its reconstruction runs behind the slice data (DecFrame::prog).
struct DecParseLaunch { int S, n, mbw, mbh, pin; const DecDesc *desc; uint64_t *prof; int K; uint32_t tag; int streamed; };  // desc: first slot
constexpr uint32_t HDR_FILL = 1024;  // RBSP bytes staged for a parameter set or slice header (the longest Baseline slice
                                     // header: 64 list-modification ops x 2 Exp-Golomb codes of <= 33 bits, ~540 bytes)
__global__ __launch_bounds__(64) void dec_hdr_kernel(DecParseLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING_BYTES];
    __shared__ DecParams ps;
    __shared__ Ring RS;
    const int lane = threadIdx.x, w = blockIdx.x;
    if (w >= a.S * a.n) return;
    const int f = w / a.S, sidx = w - f * a.S;
    const DecDesc *Dp = a.desc + w;
    DecState *st = Dp->st;
    GLOBAL DecFrame *F = uni_ptr(Dp->frm);
    const int mbw = a.mbw, mbh = a.mbh;
    if (lane == 0) ps = st->psb[a.pin];
    __syncthreads();
    Bits b;
    uint32_t refill_at = 0;
    for (int g = 0; g < f; g++) {  // parameter sets of the earlier frames of this call
        GLOBAL DecFrame *G = uni_ptr(a.desc[g * a.S + sidx].frm);
        GLOBAL const uint8_t *in = uni_ptr(G->nal);
        const int nn = uni(G->nnal);
        for (int k = 0; k < nn; k++) {
            const int type = uni(G->e[k].type);
            if (type != 7 && type != 8) continue;
            open_nal(RS, ring, in, uni(G->e[k].start), uni(G->e[k].end), b, refill_at, HDR_FILL);
            if (type == 7) parse_sps(b, ps, mbw, mbh); else parse_pps(b, ps);
        }
    }
    GLOBAL const uint8_t *in = uni_ptr(F->nal);
    const int nn = uni(F->nnal), nsl = uni(F->nsl);
    const int slice0 = nsl > 0 ? uni(F->sl[0].nal) : -1;  // the picture's first slice NAL
    const bool commit = f == a.n - 1;
    bool fail = uni(F->err) != 0;  // (an access unit without slices: no picture, no error)
    int j = 0, idr0 = 0, ref0 = 0, anyp = 0;
    for (int k = 0; k < nn; k++) {
        const int type = uni(F->e[k].type);
        const bool before = slice0 < 0 || k < slice0;
        if ((type == 7 || type == 8) && (before || commit)) {
            open_nal(RS, ring, in, uni(F->e[k].start), uni(F->e[k].end), b, refill_at, HDR_FILL);
            const bool ok = type == 7 ? parse_sps(b, ps, mbw, mbh) : parse_pps(b, ps);
            if (!ok && before) fail = true;
        } else if ((type == 1 || type == 5) && !fail) {
            // every slice header of the picture (7.4.1.2.4: its slices agree on IDR-ness and nal_ref_idc)
            open_nal(RS, ring, in, uni(F->e[k].start), uni(F->e[k].end), b, refill_at, HDR_FILL);
            const int ref_idc = (int)((uni((uint32_t)in[uni(F->e[k].start)]) >> 5) & 3);
            const SliceHdr sh = parse_slice_header(b, type, ref_idc, ps, mbw * mbh);
            if (!sh.ok) fail = true;
            if (j == 0) { idr0 = type == 5; ref0 = ref_idc != 0; }
            else if (idr0 != (type == 5) || ref0 != (ref_idc != 0)) fail = true;
            anyp |= sh.slt == 0;
            if (lane == 0) {
                GLOBAL SliceEnt *E = &F->sl[j];
                E->first_mb = sh.first_mb; E->slt = sh.slt; E->qp = sh.qp; E->data_pos = sh.data_pos; E->info = sh.info;
                E->ok = 0; E->end_mb = 0;
            }
            j++;
        }
    }
    __syncthreads();
    if (lane == 0) {
        F->got_pic = 0;
        F->hdr_ok = (!fail && nsl > 0) ? 1 : 0;
        F->anyp = anyp; F->nonref = ref0 ? 0 : 1; F->cqp = ps.cqp;
        F->sdone = 0;
        F->res_abort = 0;
        *(DecParams *)&F->ps = ps;
        if (fail && !F->err) F->err = 3;
        if (commit) st->psb[a.pin ^ 1] = ps;  // the next call's parameter sets
    }
}

// ---------------------------------------------------------------- slice-data kernel
// S * n * K waves: wave j of (frame slot, stream) parses that picture's slices j, j + K, ... (each slice
// is an independent CAVLC chain: its neighbours in other slices are unavailable, so concurrent waves
// need nothing from each other).
template <bool PROF> DEV void dec_parse_body(const DecParseLaunch &a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *ring = smem;                              // RBSP ring
    uint32_t *rows = (uint32_t *)(smem + RING_BYTES);  // mbw x {luma bottom-row TotalCoeff, chroma}
    __shared__ uint64_t s_prof[16];
    __shared__ Ring RS;
    const int K = a.K > 0 ? a.K : 1;
    const int lane = threadIdx.x, w = blockIdx.x / K, j0 = blockIdx.x - (blockIdx.x / K) * K;
    if (w >= a.S * a.n) return;
    const DecDesc *Dp = a.desc + w;
    GLOBAL DecFrame *F = uni_ptr(Dp->frm);
    GLOBAL uint64_t *prog = &F->prog;
    auto publish = [&](uint32_t rows) {
        if (lane == 0) __hip_atomic_store(prog, ((uint64_t)a.tag << 32) | rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (!uni(F->hdr_ok)) {
        if (a.streamed && j0 == 0) publish(H264MI_PROG_ABORT);  // no slice data: the reconstruction stops
        return;
    }
    const int nsl = uni(F->nsl);
    if (j0 >= nsl) return;
    // The slice chain is the decoder's longest dependency chain and shares its SIMD with wavefront
    // waves of the encoder and the reconstruction: it wins the SIMD's issue arbitration (measured:
    // the same slices parse in 17 ms alone and in 35 ms beside the encoder at normal priority).
#ifndef H264MI_PARSE_PRIO
#define H264MI_PARSE_PRIO 3
#endif
    if (H264MI_PARSE_PRIO) __builtin_amdgcn_s_setprio(H264MI_PARSE_PRIO);
    uint64_t t_prev = 0;
    uint64_t rt0 = 0, ck0 = 0;  // PROF: wall (100 MHz) and shader clock over the whole slice -> the clock the chain ran at
    if (PROF) { if (lane < 16) s_prof[lane] = 0; t_prev = clock64(); rt0 = __builtin_amdgcn_s_memrealtime(); ck0 = t_prev; }
    PT T;
    pt_load(T);
    // rows are streamed from a picture's only slice when it starts at MB 0 (else the picture's rows are
    // handed over when every slice is done)
    const int pub = a.streamed && nsl == 1 && uni(F->sl[0].first_mb) == 0 ? 1 : 0;
    int nfail = 0;
    for (int j = j0; j < nsl; j += K) {
        const int k = uni(F->sl[j].nal);
        Bits b;
        uint32_t refill_at = 0;
        open_nal(RS, ring, uni_ptr(F->nal), uni(F->e[k].start), uni(F->e[k].end), b, refill_at);
        if (PROF) { uint64_t t = clock64(); if (lane == 0) s_prof[3] += t - t_prev; t_prev = t; }
        const int slt = uni(F->sl[j].slt);
        int end_mb = 0;
        bool ok;
#define H264MI_PSD(SLT) parse_slice_data<PROF, SLT>(RS, ring, rows, refill_at, uni(F->e[k].stop), slt, uni(F->sl[j].qp), uni(F->cqp), \
                                                   uni(F->sl[j].data_pos), a.mbw, a.mbh, uni_ptr((uint32_t *)Dp->info), uni_ptr(Dp->coef), \
                                                   T, s_prof, t_prev, uni(F->sl[j].first_mb), uni(F->sl[j].info), end_mb, prog, a.tag, pub)
        if (H264MI_SLT_TEMPLATE) ok = slt == 0 ? H264MI_PSD(0) : H264MI_PSD(2);
        else ok = H264MI_PSD(-1);
#undef H264MI_PSD
        __syncthreads();
        if (lane == 0) { F->sl[j].ok = ok ? 1 : 0; F->sl[j].end_mb = end_mb; }
        nfail += ok ? 0 : 1;
    }
    __syncthreads();
    if (a.streamed) {
        // every record and slice result of this wave to memory, then count the wave done; the last of
        // the picture's waves publishes all rows, or the abort when any slice failed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int parts = nsl < K ? nsl : K;
        uint32_t old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(&F->sdone, 1u + ((uint32_t)(nfail > 0) << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
        if ((int)(old & 0xffffu) + 1 == parts)
            publish(((old >> 16) + (nfail > 0)) ? H264MI_PROG_ABORT : (uint32_t)a.mbh);
    }
    if (PROF && lane == 0) { s_prof[0] = __builtin_amdgcn_s_memrealtime() - rt0; s_prof[1] = clock64() - ck0; }
    __syncthreads();
    if (PROF && j0 == 0 && lane < 16) a.prof[w * 16 + lane] += s_prof[lane];
}
__global__ __launch_bounds__(64) void dec_parse_kernel(DecParseLaunch a) { dec_parse_body<false>(a); }
// the same kernel with section timers (H264MI_PARSE_PROF=1, tools/parse_prof.py)
__global__ __launch_bounds__(64) void dec_parse_prof_kernel(DecParseLaunch a) { dec_parse_body<true>(a); }

// Per frame, before its reconstruction: publish the slot's parse result (and the parameter sets of
// its slice) to the stream state that dec_recon_kernel / deblock_kernel and the host read.
// provisional (streamed reconstruction): the slice data may still be parsing, so only what the scan and
// header kernels decided is applied here; dec_frame_check (in dec_end_kernel) completes the decision afterwards.
// ticket: the frame's two reconstruction tickets, zeroed here (no separate memset dispatch)
// conceal / conc: slice-copy concealment is on for this call; where frame f of stream s reports its concealed MBs (conc[f * S + s])
struct DecBeginLaunch { int S, f; const DecDesc *desc; int provisional; uint32_t *ticket; int conceal; int32_t *conc; };  // desc: first slot of the call
// the picture: every slice parsed, and the slices (in any order) cover its macroblocks exactly once:
// a chain from MB 0 through first_mb -> end_mb that uses each of the nsl slices once
DEV bool slices_cover(const DecFrame *F) {
    const int nsl = F->nsl, total = F->ps.mbw * F->ps.mbh;
    int next = 0;
    for (int it = 0; it < nsl; it++) {
        int found = -1;
        for (int j = 0; j < nsl; j++)
            if (F->sl[j].first_mb == next) { found = j; break; }
        if (found < 0 || !F->sl[found].ok || F->sl[found].end_mb <= next) return false;
        next = F->sl[found].end_mb;
    }
    return next == total;
}

// ---------------------------------------------------------------- slice-copy concealment (DESIGN.md §6.5)
// dec_conceal_kernel, behind the slice data of a call and ahead of dec_resolve_kernel / the reconstruction, only
// while concealment is on: for every picture of the call that is not an IDR picture and whose good slices leave
// gaps (conceal_host.h: conceal_gaps, conceal_clean), the MB records of every gap, in dec_parse_kernel's own
// format -- P_Skip at the donor slice's QP, the synthetic slice's word (first_mb = the gap's first address, the
// donor's loop-filter fields) in dword 31 -- so that the resolve pass, the reconstruction rows and the deblocking
// rows read a picture whose lost slices were single skip runs. It also leaves the number of MBs it wrote in
// DecFrame::ncon (0: nothing to conceal, or a picture that stays rejected); whether a reference exists is the
// reconstruction side's to know, so dec_frame_begin_kernel makes the final decision from ncon.
// Work split: a block of 256 lanes per CONCEAL_SPAN MB addresses of a picture; lane t writes dword t & 31 of every
// eighth record of the gaps' part of that span (a wave instruction = two whole records, 256 contiguous bytes).
// Lane 0 of each block derives the gap table itself (<= 32 slices: a few hundred scalar steps) -- no second launch.
constexpr int CONCEAL_SPAN = 512;
struct DecConcealLaunch { int np, mbw, mbh; const DecDesc *desc; };  // desc: first slot of the call, np = frames x streams
__global__ __launch_bounds__(256) void dec_conceal_kernel(DecConcealLaunch a) {
    __shared__ int s_first[H264MI_MAX_SLICES], s_end[H264MI_MAX_SLICES], s_ok[H264MI_MAX_SLICES];
    __shared__ int s_gap[3 * H264MI_MAX_GAPS];
    __shared__ uint32_t s_rec[H264MI_MAX_GAPS][3];  // per gap: record dwords 0, 1, 31
    __shared__ int s_n;
    const int t = threadIdx.x, w = blockIdx.x, total = a.mbw * a.mbh;
    if (w >= a.np) return;
    const DecDesc &D = a.desc[w];
    DecFrame *F = D.frm;
    const int nsl = F->nsl;
    const bool cand = F->hdr_ok && !F->err && nsl > 0 && nsl <= H264MI_MAX_SLICES && F->ps.mbw == a.mbw && F->ps.mbh == a.mbh &&
                      F->e[F->sl[0].nal].type != 5;  // (the slices of a picture agree on IDR-ness: dec_hdr_kernel)
    if (cand && t < nsl) { s_first[t] = F->sl[t].first_mb; s_end[t] = F->sl[t].end_mb; s_ok[t] = F->sl[t].ok; }
    __syncthreads();
    if (t == 0) {
        int n = cand ? conceal_gaps(total, nsl, s_first, s_end, s_ok, s_gap, H264MI_MAX_GAPS) : 0;
        if (n > H264MI_MAX_GAPS || (n > 0 && !conceal_clean(total, nsl, s_first, s_end, s_ok))) n = 0;
        int mbs = 0;
        for (int g = 0; g < n; g++) {
            const SliceEnt &donor = F->sl[s_gap[3 * g + 2]];
            const int qp = donor.qp, qpc = c_CHROMA_QP[clip3(0, 51, qp + F->cqp)];
            s_rec[g][0] = MI_PSKIP | ((uint32_t)qp << 8);
            s_rec[g][1] = (uint32_t)qpc << 8;
            s_rec[g][2] = (uint32_t)s_gap[3 * g] | (donor.info & ~0xFFFFFu);
            mbs += s_gap[3 * g + 1] - s_gap[3 * g];
        }
        s_n = n > 0 ? n : 0;
        if (blockIdx.y == 0) F->ncon = n > 0 ? mbs : 0;
    }
    __syncthreads();
    const int n = s_n, lo = (int)blockIdx.y * CONCEAL_SPAN, hi = min(lo + CONCEAL_SPAN, total), dw = t & 31;
    uint32_t *info32 = (uint32_t *)D.info;
    for (int g = 0; g < n; g++) {
        const int g0 = max(s_gap[3 * g], lo), g1 = min(s_gap[3 * g + 1], hi);  // g1 <= total: inside the slot's nmb records
        const uint32_t v = dw == 0 ? s_rec[g][0] : dw == 1 ? s_rec[g][1] : dw == 31 ? s_rec[g][2] : (dw >= 2 && dw <= 5 ? 0x02020202u : 0u);
        for (int mb = g0 + (t >> 5); mb < g1; mb += 8) info32[(size_t)mb * 32 + dw] = v;
    }
}

__global__ void dec_frame_begin_kernel(DecBeginLaunch a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0 && a.ticket) { a.ticket[0] = 0; a.ticket[1] = 0; }
    if (s >= a.S) return;
    const DecDesc &D = a.desc[a.f * a.S + s];
    DecState *st = D.st;
    const DecFrame *F = D.frm;
    if (F->hdr_ok) st->ps = F->ps;
    bool ok = F->hdr_ok && !F->err;
    int ncon = 0;  // MBs concealed: the good slices leave gaps, dec_conceal_kernel filled them, and a reference exists
    if (ok && !a.provisional) {
        const bool cover = slices_cover(F);
        if (!cover && a.conceal && F->ncon > 0 && st->has_ref) ncon = F->ncon;
        ok = (cover || ncon > 0) && !F->res_abort;
    }
    // a P slice with no earlier decoded picture (no reference) yields no picture, like a parse error
    if (ok && F->anyp && !st->has_ref) ok = false;
    st->got_pic = ok ? 1 : 0;
    st->nonref = F->nonref;
    // per frame: a damaged access unit yields no picture, the next one decodes (no slices at all: no error)
    st->err = ok ? 0 : (F->err ? F->err : (F->hdr_ok ? (F->res_abort ? 1 : 3) : 0));
    if (ok) st->epoch = st->epoch + 1;
    if (a.conc) a.conc[a.f * a.S + s] = ok ? ncon : 0;
}
// Streamed reconstruction, after dec_recon_kernel (and after the slice data of the call is parsed): the
// picture stands only if its slices cover it and the wavefront was not aborted; otherwise it is
// concealed like any damaged access unit (pic[parity ^ 1], which the speculative rows wrote, is neither
// output nor made the reference). Runs inside dec_end_kernel (dec_recon.inc).
DEV void dec_frame_check(const DecDesc &D) {
    DecState *st = D.st;
    const DecFrame *F = D.frm;
    if (!st->got_pic) return;
    const bool cover = slices_cover(F);
    if (st->err == 0 && cover) return;
    st->got_pic = 0;
    st->err = cover ? 1 : (F->err ? F->err : 3);  // 1: the wavefront aborted on a whole picture
}

}  // namespace h264mi
