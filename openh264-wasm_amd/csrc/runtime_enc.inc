// runtime_enc.inc -- host runtime of the encoder: HBM allocation, per-frame launch sequence,
// parameter-set generation. Lives in the kernels' translation unit so launches see the kernels.
// The stages in front of the frame step: their state is EncInput here, their logic enc_input.inc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "picture_host.h"  // what quality.hip, scale.hip, compose.hip, overlay.hip and upscale.hip export, and the shared host rules

namespace h264mi {

#define HIPCHECK(x)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "h264mi: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -1;                                                                                \
        }                                                                                             \
    } while (0)

// ---------------------------------------------------------------- host bit writer (parameter sets only)
struct HostBits {
    std::vector<uint8_t> b;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t v, int k) {
        if (k <= 0) return;
        if (k < 32) v &= (1u << k) - 1u;
        acc = (acc << k) | v; n += k;
        while (n >= 8) { n -= 8; b.push_back((uint8_t)(acc >> n)); }
    }
    void ue(uint32_t v) { uint64_t k = (uint64_t)v + 1; int l = 0; while ((k >> l) > 1) l++; put(0, l); put((uint32_t)k, l + 1); }
    void se(int v) { ue(v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }
    void trailing() { put(1, 1); if (n) put(0, 8 - n); }
};
static size_t nal_wrap(uint8_t *out, int ref_idc, int type, const std::vector<uint8_t> &rbsp) {
    size_t o = 0;
    out[o++] = 0; out[o++] = 0; out[o++] = 0; out[o++] = 1;
    out[o++] = (uint8_t)((ref_idc << 5) | type);
    int z = 0;
    for (uint8_t c : rbsp) {
        if (z >= 2 && c <= 3) { out[o++] = 3; z = 0; }
        out[o++] = c;
        z = c == 0 ? z + 1 : 0;
    }
    return o;
}
// OpenH264's level choice (WelsInitSps, h264.wasm func 280; oracle h264o_level_idc, DESIGN.md §3.1): the
// first row of g_ksLevelLimits {idc, MaxMBPS, MaxFS, MaxDpbMbs, MaxBR} (the binary's order) covering the MB
// rate at 60 fps, the frame size, max(mbw^2, mbh^2) <= 8 MaxFS, the DPB (1 reference) and the bitrate
// (MaxBR * 1200); none: 51; level 1b -> idc 11 with constraint_set3.
static int level_idc_for(int w, int h, int bitrate, int *cs3) {
    static const int32_t L[17][5] = {
        {10, 1485, 99, 396, 64},       {9, 1485, 99, 396, 128},       {11, 3000, 396, 900, 192},
        {12, 6000, 396, 2376, 384},    {13, 11880, 396, 2376, 768},   {20, 11880, 396, 2376, 2000},
        {21, 19800, 792, 4752, 4000},  {22, 20250, 1620, 8100, 4000}, {30, 40500, 1620, 8100, 10000},
        {31, 108000, 3600, 18000, 14000}, {32, 216000, 5120, 20480, 20000}, {40, 245760, 8192, 32768, 20000},
        {41, 245760, 8192, 32768, 50000}, {42, 522240, 8704, 34816, 50000}, {50, 589824, 22080, 110400, 135000},
        {51, 983040, 36864, 184320, 240000}, {52, 2073600, 36864, 184320, 240000}};
    const uint32_t mbw = (uint32_t)(w + 15) >> 4, mbh = (uint32_t)(h + 15) >> 4, mbs = mbw * mbh;
    const uint32_t sq = mbw * mbw > mbh * mbh ? mbw * mbw : mbh * mbh;
    const uint32_t mbps = (uint32_t)(60.0f * (float)mbs);
    int level = 51;
    *cs3 = 0;
    for (auto &l : L) {
        if ((uint32_t)l[1] < mbps || (uint32_t)l[2] < mbs || ((uint32_t)l[2] << 3) < sq || (uint32_t)l[3] < mbs) continue;
        if (bitrate && l[4] * 1200 < bitrate) continue;
        level = l[0];
        break;
    }
    if (level == 9) { *cs3 = 1; level = 11; }
    return level;
}
// OpenH264's SPS (WelsInitSps + WelsWriteSpsSyntax / WelsWriteVUI, h264.wasm funcs 280 / 640; DESIGN.md
// §3.1): Baseline, constraint_set0/1, log2_max_frame_num 15, POC type 2, 1 reference, direct_8x8_inference
// from level 3.0, cropping, VUI with only bitstream_restriction (mv over boundaries, log2 max mv length 16,
// 0 reorder frames, 1 frame buffering).
static size_t write_sps(int w, int h, int bitrate, uint8_t *out) {
    int mbw = (w + 15) / 16, mbh = (h + 15) / 16, cs3;
    const int level = level_idc_for(w, h, bitrate, &cs3);
    HostBits b;
    b.put(66, 8); b.put(0xC0 | (cs3 << 4), 8); b.put(level, 8);
    b.ue(0); b.ue(15 - 4); b.ue(2); b.ue(1); b.put(0, 1);
    b.ue(mbw - 1); b.ue(mbh - 1); b.put(1, 1); b.put(level >= 30, 1);
    int crop = (mbw * 16 != w) || (mbh * 16 != h);
    b.put(crop, 1);
    if (crop) { b.ue(0); b.ue((mbw * 16 - w) / 2); b.ue(0); b.ue((mbh * 16 - h) / 2); }
    b.put(1, 1);                                  // vui_parameters_present_flag
    b.put(0, 8);                                  // aspect, overscan, signal type, chroma loc, timing, hrd x2, pic_struct
    b.put(1, 1); b.put(1, 1);                     // bitstream_restriction, motion_vectors_over_pic_boundaries
    b.ue(0); b.ue(0); b.ue(16); b.ue(16); b.ue(0); b.ue(1);
    b.trailing();
    return nal_wrap(out, 3, 7, b.b);
}
static size_t write_pps(uint8_t *out) {
    HostBits b;
    b.ue(0); b.ue(0); b.put(0, 1); b.put(0, 1); b.ue(0); b.ue(0); b.ue(0); b.put(0, 1); b.put(0, 2);
    b.se(0); b.se(0); b.se(0); b.put(1, 1); b.put(0, 1); b.put(0, 1);
    b.trailing();
    return nal_wrap(out, 3, 8, b.b);
}
// OpenH264's rate-control constants at the wrapper's parameters (DESIGN.md §3.6; oracle rc_init /
// rc_update_bitrate_fps / rc_idr_class, restated from the reference's h264.wasm): RcInitSequenceParameter (func 592,
// iRcVaryPercentage 10: GOMs of 2 MB rows from 31 MBs wide, iSkipQpValue 24 / 31), RcInitTlWeight (func 702: one
// temporal layer, weight 2000, VGOP of 8 frames), RcUpdateBitrateFps (func 697: float bits per frame at the default
// 60 fps, the layer's bits bounds 55 % / 150 %, skip buffer 50 % of the bitrate) and RcCalculateIdrQp's table part
// (func 1226: the layer's size rounded to whole MBs by ParamTranscode, func 585; bpp class and column; the IDR QP
// range clipped to the camera range [12, 42]; the first IDR's QP). Tables: tests/golden/openh264_tables.json.
static void rc_seq_init(RcState &r, int w, int h, int bitrate) {
    static const double BPP[4][4] = {{0.25, 0.5, 0.75, 1.0}, {0.1, 0.2, 0.3, 0.4}, {0.03, 0.05, 0.09, 0.13}, {0.01, 0.03, 0.06, 0.1}};
    static const int INITQP[4][5] = {{34, 28, 26, 24, 22}, {36, 30, 28, 26, 24}, {36, 32, 30, 28, 26}, {36, 34, 32, 30, 28}};
    static const int RANGE[5][2] = {{40, 28}, {37, 25}, {36, 24}, {35, 23}, {34, 22}};
    auto clip = [](int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); };
    memset(&r, 0, sizeof(r));
    const int w16 = (w + 15) & ~15, h16 = (h + 15) & ~15;
    r.mbw = w16 >> 4;
    r.nmb = r.mbw * (h16 >> 4);
    const bool narrow = r.mbw < 31;
    const int g0 = narrow ? 1 : 2, g1 = narrow ? 2 : 4;
    r.skip_qp = narrow ? 24 : 31;
    r.mb_per_gom = r.mbw * ((10 * (g1 - g0)) / 100 + g0);
    r.gom_count = (r.mb_per_gom + r.nmb - 1) / r.mb_per_gom;
    r.tl_weight = 2000;
    r.gop_num = 8;
    const float fps = 60.0f;
    r.c_bpf = (int)((fps * 0.5f + (float)bitrate) / fps);
    r.c_max_bits_tl = (int)(((int64_t)r.c_bpf * 150 * r.tl_weight + 100000) / 200000);
    r.c_min_bits_tl = (int)(((int64_t)r.c_bpf * (100 - ((100 - 10) >> 1)) * r.tl_weight + 100000) / 200000);
    r.c_buffer_size_skip = (int)((50 * (int64_t)bitrate + 50) / 100);
    const double bpp = (double)bitrate / (double)((fps * (float)w16) * (float)h16);
    const int area = w16 * h16;
    const int cls = area < 28801 ? 0 : ((unsigned)area < 115201u ? 1 : ((unsigned)area < 460801u ? 2 : 3));
    int i = 0;
    while (i < 4 && !(BPP[cls][i] >= bpp)) i++;
    r.idr_hi = clip(12, 42, RANGE[i][0]);
    r.idr_lo = clip(12, 42, RANGE[i][1]);
    r.idr_table_qp = INITQP[cls][i];
    r.skip_en = 1;  // the wrapper leaves OpenH264's frame skipping on
}

// GPU-side wait budget (h264mi_dev.h WaitClock) from H264MI_WAIT_LIMIT_MS, applied when an encoder or a decoder
// is created; unset: the compiled default (2 s)
static void wait_limit_from_env() {
    const char *e = getenv("H264MI_WAIT_LIMIT_MS");
    if (!e) return;
    const long ms = atol(e);
    if (ms <= 0) return;
    const uint64_t ticks = (uint64_t)ms * 100000u;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wait_limit_ticks), &ticks, sizeof(ticks));
}

// ---------------------------------------------------------------- encoder context
// The stages an encoder runs on its input area in front of the frame step, in the order they run (enc_input.inc holds
// the chain, the setters and the release; DESIGN.md §5.16). Each holds its parameters p, whether it is on, its device
// state -- allocated when the stage is turned on, freed when it is turned off -- and whether that state holds a frame
// yet. Every stage off: a frame step enqueues what it did before the stages existed
struct EncInput {
    struct Deinterlace {  // h264mi_enc_set_deinterlace; deinterlace.hip
        bool on = false, has = false; h264mi_deinterlace p = {};
        uint8_t *d_prev = nullptr;  // the S previous unfiltered frames
    } di;
    struct Denoise {  // the pre-filter: h264mi_enc_set_denoise; denoise.hip
        bool on = false, has = false; h264mi_denoise p = {};
        uint8_t *d_prev = nullptr;  // the S previous filtered frames
    } dn;
    struct Levels {  // the levels stage: h264mi_enc_set_levels; levels.hip. The state's first word is the stream's `has`
        bool on = false; h264mi_levels p = {};
        uint8_t *d_mem = nullptr;  // per stream 768 histogram words, then 768 table bytes, 4 state words, 8 record words
        uint32_t *hist() const { return (uint32_t *)d_mem; }
        uint8_t *luts(int S) const { return d_mem + (size_t)S * 3072; }
        int32_t *state(int S) const { return (int32_t *)(d_mem + (size_t)S * 3840); }
        int32_t *record(int S) const { return (int32_t *)(d_mem + (size_t)S * 3856); }
        static size_t bytes(int S) { return (size_t)S * 3888; }
    } lv;
    struct Spatial {  // the sharpen/blur filter: h264mi_enc_set_spatial; spatial.hip
        bool on = false; h264mi_spatial p = {};
        uint8_t *d_buf = nullptr;  // the S frames it filters into: what the later stages and the frame step work on
    } sp;
    struct Privacy {  // h264mi_enc_set_privacy; spatial.hip: host copies of the masks, frame = stream
        std::vector<h264mi_privacy> list;  // empty: off
    } pv;
    struct Scenecut {  // the key-frame policy: h264mi_enc_set_scenecut; scenecut.hip
        bool on = false, has = false; h264mi_scenecut p = {};
        uint32_t *d_words = nullptr;  // per stream sixteen words, then per stream eight statistics words: 24 S words
        uint8_t *d_thumb = nullptr;   // the S thumbnails, only with share > 0; has speaks of them
    } sc;
    struct Overlays {  // h264mi_enc_set_overlays; overlay.hip: host copies of the placements, the caller's sprites
        std::vector<h264mi_overlay> list;  // empty: off
        const uint8_t *sprites = nullptr;
        int w = 0, h = 0;  // the sprites' size
    } ov;
    bool any() const { return di.on || dn.on || lv.on || sp.on || !pv.list.empty() || sc.on || !ov.list.empty(); }
};

struct EncCtx {
    int w, h, mbw, mbh, nmb, cw, ch, S, bitrate;
    hipStream_t stream;
    bool own_stream;

    size_t fbytes;            // tight I420 bytes per frame
    uint8_t *d_src = nullptr; // S frames (host-input path)
    uint8_t *d_pool = nullptr;
    EncState *d_st = nullptr;
    EncDesc *d_desc[2] = {nullptr, nullptr};
    DbkDesc *d_dbk[2] = {nullptr, nullptr};
    PlanesDesc *d_pd[2] = {nullptr, nullptr};  // motion-search planes built from the frame of that parity
    uint32_t *d_ticket = nullptr;
    uint32_t *d_done = nullptr;  // enc_begin_kernel's per-stream workgroup counters
    int gom_count = 0, begin_k = 1;  // GOMs per picture, enc_begin_kernel's workgroups per stream
    int gom_rows = 1;            // MB rows per GOM (RcInitSequenceParameter)
    int sgrp = 0;                // enc_mb_kernel: streams per ticket group of a queue (EncLaunch::sgrp; 0: all)
    bool gom_exact = false;      // OpenH264's GOM QP rule (h264mi_enc_set_gom_exact; enc_bits.inc gom_row_qp)
    int slices = 1;              // slices per picture from the next frame step on (h264mi_enc_set_slices; BeginLaunch::slices)
    bool quality = false;        // per-frame distortion records from the next frame step on (h264mi_enc_set_quality)
    h264mi_quality *d_qual = nullptr;  // S records (quality.hip), allocated when the option is first turned on: an
                                       // encoder that never uses it holds exactly the memory it held before
    std::vector<EncDesc> h_desc[2];
    int parity = 0;
    // host-side output staging (C-ABI path)
    std::vector<uint8_t> h_out;
    // optional HIP-event timing of the dominant kernel (enc_mb_kernel), for bench.py's roofline
    bool timing = false;
    uint64_t *d_prof = nullptr;  // enc_mb_kernel section counters (env H264MI_ENC_PROF=1)
    uint64_t *d_tl = nullptr;    // enc_mb_kernel per-ticket {start, end} timeline of the last frame (env H264MI_ENC_TL=1)
    int dlag = 0;                // deblocking rows' ticket lag (EncLaunch::dlag; env H264MI_DBK_LAG)
    int prio = 0;                // encoder rows' wave priority (EncLaunch::prio; env H264MI_ENC_PRIO)
    int prof_row = -1;           // section counters of one MB row only (EncLaunch::prof_row; env H264MI_ENC_PROF_ROW)
    int lean = -1;               // enc_mb_kernel build: 1 occupancy target, 0 unconstrained, -1 by launch size
    // per-XCD ticket queues when S % 8 == 0 (env H264MI_ENC_XQ=0 turns them off): a stream's MB rows all run on
    // one XCD, so the four rows that read each reference-window row meet in that XCD's L2 -- the launch's HBM
    // traffic falls from 22.7x to 7.3x algorithmic at 32 streams with throughput within noise (-1 % at 32
    // streams, +0.3-1 % at 64 / 128; profiles/round5/ab_xq*.txt; round 3 measured 0.5-1 % slower and left them off)
    int xq = 1;
    int ncu = 256;               // the device's CUs (enc_frame's build choice)
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    // what h264mi_enc_encode_rgba converts under (h264mi_enc_set_colorspec; colorspace.hip). All 0: the wrapper's
    // conversion by color.inc's kernel, as before the specification existed
    h264mi_colorspec cs = {};
    h264mi_pixopt pixopt = {};   // the depth rule h264mi_enc_encode_pix converts 10-bit layouts under (h264mi_enc_set_pixopt)
    EncInput in;                 // the stages in front of the frame step (above; their logic: enc_input.inc)
};

struct EncMbLaunch {  // enc_mb_kernel reads the source frames through this launch-time base
    const uint8_t *src_base;
    size_t src_stride;
};

static void enc_input_release(EncCtx *c);  // enc_input.inc

static void enc_free(EncCtx *c) {
    if (!c) return;

    for (auto e : c->ev) (void)hipEventDestroy(e);
    (void)hipFree(c->d_pool);
    (void)hipFree(c->d_qual);
    enc_input_release(c);
    (void)hipFree(c->d_prof);
    (void)hipFree(c->d_tl);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Per-frame distortion records (DESIGN.md §5.2): one host flag; a frame step issued while it is set appends
// quality_kernel on the encoder's stream. Turning it on clears the records (in stream order), so that what is read
// before the next step says "nothing coded" instead of showing an earlier frame's figures
static int enc_set_quality(EncCtx *c, bool on) {
    if (c->w < 16 || c->h < 16) return -1;
    if (on && !c->quality) {
        if (!c->d_qual && hipMalloc(&c->d_qual, sizeof(h264mi_quality) * (size_t)c->S) != hipSuccess) { c->d_qual = nullptr; return -1; }
        if (hipMemsetAsync(c->d_qual, 0, sizeof(h264mi_quality) * (size_t)c->S, c->stream) != hipSuccess) return -1;
    }
    c->quality = on;
    return 0;
}

// a picture of mbh MB rows can be coded as n slices of whole MB rows (h264mi_dev.h slice_first_row)
static bool slices_valid(int mbh, int n) { return n >= 1 && n <= mbh && n <= H264MI_MAX_SLICES; }

static EncCtx *enc_create(int w, int h, int bitrate, int S, hipStream_t stream) {
    // h <= 4096: at most 256 MB rows (the pack kernel's row table)
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || S <= 0 || S > H264MI_MAX_STREAMS || w > 16 * H264MI_ENC_MAX_MBW || h > 4096) return nullptr;
    wait_limit_from_env();
    EncCtx *c = new EncCtx();
    c->w = w; c->h = h; c->mbw = (w + 15) / 16; c->mbh = (h + 15) / 16; c->nmb = c->mbw * c->mbh;
    c->cw = c->mbw * 16; c->ch = c->mbh * 16; c->S = S; c->bitrate = bitrate;
    c->fbytes = (size_t)w * h + 2 * (size_t)(w / 2) * (h / 2);
    if (stream) { c->stream = stream; c->own_stream = false; }
    else { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return nullptr; } c->own_stream = true; }
    const size_t ysz = (size_t)c->cw * c->ch, csz = ysz / 4, pic = ysz + 2 * csz;
    const size_t rbsp_dw = (size_t)c->nmb * H264MI_MB_SLOT_DWORDS + 1024;
    const size_t nal_cap = rbsp_dw * 4 * 3 / 2 + 4096;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // per-stream layout
    size_t off_rec = 0, off_ref0 = off_rec + al(pic), off_ref1 = off_ref0 + al(pic);
    size_t off_info = off_ref1 + al(pic), off_coef = off_info + al(sizeof(MbInfo) * c->nmb);
    size_t off_gran = off_coef + al(sizeof(MbCoef) * c->nmb);
    size_t off_dgran = off_gran + al(8 * (size_t)H264MI_GRANULES_PER_MB * c->nmb);
    size_t off_bits = off_dgran + al(8 * (size_t)H264MI_DBK_GRANULES_PER_MB * c->nmb);
    size_t off_len = off_bits + al(4 * (size_t)H264MI_MB_SLOT_DWORDS * c->nmb);
    size_t off_rbsp = off_len + al(4 * (size_t)c->nmb);
    size_t off_nal = off_rbsp + al(4 * rbsp_dw);
    const size_t lps = (size_t)c->cw + 2 * H264MI_LPADX, lph = (size_t)c->ch + 2 * H264MI_LPADY;
    const size_t cps = (size_t)c->cw / 2 + 2 * H264MI_CPADX, cph = (size_t)c->ch / 2 + 2 * H264MI_CPADY;
    size_t off_pl = off_nal + al(nal_cap), off_plc = off_pl + 4 * al(lps * lph);
    size_t off_egr = off_plc + 2 * al(cps * cph);
    size_t off_rowqp = off_egr + al(8 * 128 * (size_t)c->nmb), off_rowbits = off_rowqp + al(4 * (size_t)c->mbh);
    size_t off_rowq = off_rowbits + al(4 * (size_t)c->mbh);
    // defaults for new encoders: exact GOM mode, then the slice count (a bad value, or one with exact GOM, is ignored)
    if (const char *e = getenv("H264MI_GOM_EXACT")) c->gom_exact = atoi(e) != 0;
    if (const char *e = getenv("H264MI_ENC_SLICES")) {
        const int n = atoi(e);
        if (slices_valid(c->mbh, n) && !(c->gom_exact && n > 1)) c->slices = n;
    }
    RcState rc0;
    rc_seq_init(rc0, w, h, bitrate);
    c->gom_count = rc0.gom_count;
    c->begin_k = rc0.gom_count < 8 ? rc0.gom_count : 8;
    size_t off_psrc = off_rowq + al(8 * (size_t)c->mbh), off_gomc = off_psrc + 2 * al(ysz);
    size_t off_bitg = off_gomc + al(8 * (size_t)rc0.gom_count), off_gomst = off_bitg + al(8 * (size_t)c->nmb);
    size_t off_sks = off_gomst + al(32 * (size_t)rc0.gom_count);
    size_t per = off_sks + 2 * al(4 * ((size_t)c->nmb + 1));
    c->gom_rows = rc0.mb_per_gom / rc0.mbw;
    size_t hdr = al(sizeof(EncState) * S) + 2 * al(sizeof(EncDesc) * S) + 2 * al(sizeof(DbkDesc) * S) + 2 * al(sizeof(PlanesDesc) * S) + 256 + al(4 * (size_t)S);
    size_t total = hdr + al(c->fbytes * S) + per * S;
    if (hipMalloc(&c->d_pool, total) != hipSuccess) { if (c->own_stream) (void)hipStreamDestroy(c->stream); delete c; return nullptr; }
    (void)hipMemsetAsync(c->d_pool, 0, total, c->stream);
    uint8_t *p = c->d_pool;
    c->d_st = (EncState *)p; p += al(sizeof(EncState) * S);
    c->d_desc[0] = (EncDesc *)p; p += al(sizeof(EncDesc) * S);
    c->d_desc[1] = (EncDesc *)p; p += al(sizeof(EncDesc) * S);
    c->d_dbk[0] = (DbkDesc *)p; p += al(sizeof(DbkDesc) * S);
    c->d_dbk[1] = (DbkDesc *)p; p += al(sizeof(DbkDesc) * S);
    c->d_pd[0] = (PlanesDesc *)p; p += al(sizeof(PlanesDesc) * S);
    c->d_pd[1] = (PlanesDesc *)p; p += al(sizeof(PlanesDesc) * S);
    c->d_ticket = (uint32_t *)p; p += 256;
    c->d_done = (uint32_t *)p; p += al(4 * (size_t)S);
    c->d_src = p; p += al(c->fbytes * S);
    std::vector<EncState> hs(S);
    std::vector<DbkDesc> hd[2];
    std::vector<PlanesDesc> hp[2];
    uint8_t sps[64], pps[32];
    size_t nsps = write_sps(w, h, bitrate, sps), npps = write_pps(pps);
    for (int par = 0; par < 2; par++) { c->h_desc[par].resize(S); hd[par].resize(S); hp[par].resize(S); }
    for (int s = 0; s < S; s++) {
        uint8_t *b = p + per * s;
        uint8_t *rec = b + off_rec, *r0 = b + off_ref0, *r1 = b + off_ref1;
        for (int par = 0; par < 2; par++) {
            EncDesc &d = c->h_desc[par][s];
            uint8_t *ref = par == 0 ? r0 : r1, *dbk = par == 0 ? r1 : r0;
            d.src = nullptr;
            d.rec[0] = rec; d.rec[1] = rec + ysz; d.rec[2] = rec + ysz + csz;
            d.ref[0] = ref; d.ref[1] = ref + ysz; d.ref[2] = ref + ysz + csz;
            d.dbk[0] = dbk; d.dbk[1] = dbk + ysz; d.dbk[2] = dbk + ysz + csz;
            d.info = (MbInfo *)(b + off_info); d.coef = (MbCoef *)(b + off_coef);
            d.gran = (uint64_t *)(b + off_gran); d.dgran = (uint64_t *)(b + off_dgran);
            d.mbbits = (uint32_t *)(b + off_bits); d.mblen = (uint32_t *)(b + off_len);
            d.rbsp = (uint32_t *)(b + off_rbsp); d.nal = b + off_nal;
            d.st = c->d_st + s; d.nal_cap = (int)nal_cap; d.rbsp_cap = (int)rbsp_dw;
            for (int k = 0; k < 4; k++) d.pl[k] = b + off_pl + k * al(lps * lph) + H264MI_LPADY * lps + H264MI_LPADX;
            for (int k = 0; k < 2; k++) d.plc[k] = b + off_plc + k * al(cps * cph) + H264MI_CPADY * cps + H264MI_CPADX;
            d.ps = (int)lps; d.psc = (int)cps; d.pad3[0] = d.pad3[1] = 0;
            d.egran = (uint64_t *)(b + off_egr);
            d.rowqp = (int32_t *)(b + off_rowqp); d.rowbits = (int32_t *)(b + off_rowbits); d.rowq = (uint64_t *)(b + off_rowq);
            d.psrc[0] = b + off_psrc; d.psrc[1] = b + off_psrc + al(ysz);
            d.gomc = (uint32_t *)(b + off_gomc);
            d.bitg = (uint64_t *)(b + off_bitg); d.gomst = (uint64_t *)(b + off_gomst);
            int32_t *sk0 = (int32_t *)(b + off_sks), *sk1 = (int32_t *)(b + off_sks + al(4 * ((size_t)c->nmb + 1)));
            d.sksad_ref = par == 0 ? sk0 : sk1; d.sksad_cur = par == 0 ? sk1 : sk0;
            DbkDesc &k = hd[par][s];
            for (int i = 0; i < 3; i++) { k.rec[i] = d.rec[i]; k.out[0][i] = d.dbk[i]; k.out[1][i] = d.dbk[i]; }
            k.info = d.info; k.dgran = d.dgran; k.epoch = &c->d_st[s].epoch; k.disable = nullptr;
            k.active = nullptr; k.parity = nullptr; k.abort_word = &c->d_st[s].err; k.src_gran = d.egran;
            PlanesDesc &pd = hp[par][s];
            for (int i = 0; i < 3; i++) pd.src[0][i] = pd.src[1][i] = d.dbk[i];
            pd.parity = nullptr; pd.active = nullptr;
            for (int k2 = 0; k2 < 4; k2++) pd.pl[k2] = d.pl[k2];
            pd.plc[0] = d.plc[0]; pd.plc[1] = d.plc[1]; pd.ps = d.ps; pd.psc = d.psc;
        }
        EncState &st = hs[s];
        memset(&st, 0, sizeof(st));
        st.rc = rc0;
        st.first = 1; st.idr_pic_id = 0; st.bitrate = bitrate;  // first IDR: 1 (DESIGN.md §3.1)
        st.cur_slices = c->slices;
        // the first frame's MB-row QP plan: no rows coded yet, every row at the frame QP (offset 0)
        std::vector<int32_t> rq((size_t)c->mbh, 0);
        (void)hipMemcpyAsync(b + off_rowqp, rq.data(), 4 * (size_t)c->mbh, hipMemcpyHostToDevice, c->stream);
        (void)hipStreamSynchronize(c->stream);
        st.sps_bytes = (int)nsps; st.pps_bytes = (int)npps;
        memcpy(st.sps, sps, nsps); memcpy(st.pps, pps, npps);
    }
    (void)hipMemcpyAsync(c->d_st, hs.data(), sizeof(EncState) * S, hipMemcpyHostToDevice, c->stream);
    for (int par = 0; par < 2; par++) {
        (void)hipMemcpyAsync(c->d_desc[par], c->h_desc[par].data(), sizeof(EncDesc) * S, hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(c->d_dbk[par], hd[par].data(), sizeof(DbkDesc) * S, hipMemcpyHostToDevice, c->stream);
        (void)hipMemcpyAsync(c->d_pd[par], hp[par].data(), sizeof(PlanesDesc) * S, hipMemcpyHostToDevice, c->stream);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { enc_free(c); return nullptr; }
    if (const char *e = getenv("H264MI_DBK_LAG")) c->dlag = atoi(e);
    if (const char *e = getenv("H264MI_ENC_PRIO")) c->prio = atoi(e);
    if (const char *e = getenv("H264MI_ENC_PROF_ROW")) c->prof_row = atoi(e);
    if (const char *e = getenv("H264MI_ENC_LEAN")) c->lean = atoi(e);  // diagnostics: force a build
    if (const char *e = getenv("H264MI_ENC_XQ")) c->xq = atoi(e);      // A/B: ticket queues
    if (const char *e = getenv("H264MI_ENC_SGRP")) c->sgrp = atoi(e);               // A/B: streams per ticket group
    {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            c->ncu = n;
    }
    if (const char *e = getenv("H264MI_ENC_QUALITY")) (void)enc_set_quality(c, atoi(e) != 0);  // refused below 16x16
    if (getenv("H264MI_ENC_TL") && hipMalloc(&c->d_tl, 4 * (size_t)S * c->mbh * sizeof(uint64_t)) == hipSuccess)
        (void)hipMemset(c->d_tl, 0, 4 * (size_t)S * c->mbh * sizeof(uint64_t));
    if (getenv("H264MI_ENC_PROF") && hipMalloc(&c->d_prof, 64 * sizeof(uint64_t)) == hipSuccess)
        (void)hipMemset(c->d_prof, 0, 64 * sizeof(uint64_t));  // 0..15 + 32..51 enc_mb_kernel, 16..21 deblocking rows
    return c;
}

// One frame step for all S streams. src: S tight I420 frames, contiguous, in device memory.
static int enc_frame(EncCtx *c, const uint8_t *d_frames) {
    const int par = c->parity;
    const int src_vec = (c->w % 16) == 0 && (c->fbytes % 16) == 0 && ((uintptr_t)d_frames % 16) == 0;
    // frame complexity + skip decision + the rate control's picture init (enc_bits.inc)
    hipLaunchKernelGGL(enc_begin_kernel, dim3(c->begin_k, c->S), dim3(256), 0, c->stream,
                       BeginLaunch{c->S, c->w, c->h, c->cw, c->ch, c->begin_k, c->d_desc[par], c->d_ticket, d_frames, c->fbytes, src_vec, c->d_done, c->slices});
    EncLaunch el{c->w, c->h, c->mbw, c->mbh, c->S, c->d_desc[par], c->d_ticket, d_frames, c->fbytes, c->d_prof, src_vec,
                 c->d_dbk[par], c->d_prof ? c->d_prof + 16 : nullptr, c->dlag};
    if (c->timing) {
        if (c->ev_used + 2 > (int)c->ev.size()) {
            for (int i = 0; i < 64; i++) { hipEvent_t e; HIPCHECK(hipEventCreate(&e)); c->ev.push_back(e); }
        }
        HIPCHECK(hipEventRecord(c->ev[c->ev_used], c->stream));
    }
    // MB-row encoders and the deblocking rows that trail them, one launch (enc_mb_kernel)
    // the occupancy-target build once the encoder rows exceed two workgroups per CU (the unconstrained
    // build's residency): 1080p x 8 streams = 544 rows -> lean, 720p x 8 = 360 and 1080p x 4 -> not
    const bool lean = c->lean >= 0 ? c->lean != 0 : c->S * c->mbh >= 2 * c->ncu;
    // per-XCD ticket queues: streams a multiple of 8, in-order deblocking tickets (dlag 0)
    if (c->xq != 0 && c->S % 8 == 0 && (c->dlag <= 0 || c->gom_exact)) el.xq = 8;
    el.tl = c->d_tl;
    el.prio = c->prio;
    el.prof_row = c->prof_row;
    if (c->gom_exact) { el.gomr = c->gom_rows; el.dlag = 0; }
    el.sgrp = c->sgrp;
    if (lean) hipLaunchKernelGGL(enc_mb_kernel<true>, dim3(2 * c->S * c->mbh), dim3(ENC_THREADS), 0, c->stream, el);
    else hipLaunchKernelGGL(enc_mb_kernel<false>, dim3(2 * c->S * c->mbh), dim3(ENC_THREADS), 0, c->stream, el);
    if (c->timing) { HIPCHECK(hipEventRecord(c->ev[c->ev_used + 1], c->stream)); c->ev_used += 2; }
    // the slices' packing (and the rate control) and the next frame's motion-search planes from this
    // frame's deblocked picture, one launch (enc_post_kernel). (The planes on a side stream beside the
    // packing were measured slower twice: 1715 -> 1312 frames/s in round 1 with 4 hardware queues,
    // 1315 -> 1249 in round 2 with 8.)
    // (the pack of a multi-slice frame is a kernel of its own: c->slices is what this step's begin kernel latches)
    if (launch_enc_post(PackLaunch{c->mbw, c->mbh, c->S, c->d_desc[par]}, c->cw, c->ch, c->d_pd[par], c->stream, c->slices > 1) != 0) return -1;
    HIPCHECK(hipGetLastError());
    // the frame's distortion, behind the pack (its NAL byte counts) and the deblocking rows: the source against the
    // display area of this parity's deblocked pictures (quality.hip)
    if (c->quality && launch_quality_enc(c->d_qual, d_frames, c->fbytes, c->w, c->h, c->cw, c->d_desc[par], c->S, c->stream) != 0) return -1;
    c->parity ^= 1;
    return 0;
}

}  // namespace h264mi

namespace h264mi {
// copy every stream's NAL output into fixed slots of a caller buffer (device), sizes from EncState
struct PackNalLaunch { int S; const EncDesc *desc; uint8_t *dst; int slot; int32_t *sizes; };
__global__ __launch_bounds__(256) void enc_copy_nals_kernel(PackNalLaunch a) {
    const int s = blockIdx.y;
    if (s >= a.S) return;
    const EncDesc &D = a.desc[s];
    int n = D.st->nal_bytes;
    if (n > a.slot) { if (blockIdx.x == 0 && threadIdx.x == 0) D.st->err = 4; n = a.slot; }
    if (a.sizes && blockIdx.x == 0 && threadIdx.x == 0) a.sizes[s] = n;
    uint8_t *o = a.dst + (size_t)s * a.slot;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) *(uint32_t *)(o + i) = *(const uint32_t *)(D.nal + i);
        else for (int k = i; k < n; k++) o[k] = D.nal[k];
    }
}
}  // namespace h264mi
