/*
 * oracle/h264o_api.h -- TEST INFRASTRUCTURE ONLY. The CPU oracle's C API (loaded by tests/ via
 * ctypes, by __graft_entry__.smoke() as the checker, and by bench.py's cpu_baseline leg). The
 * product library (openh264-wasm_amd/, include/h264mi.h) never includes or links this.
 *
 * Parity status: the encoder restates OpenH264's algorithm at the wrapper's parameters but is
 * "parity unpinned" against OpenH264 itself (no reference tests, fixtures or runnable build --
 * see DESIGN.md §3); the decoder restates the normative H.264 decoding process.
 */
#ifndef H264O_API_H
#define H264O_API_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct H264OEnc H264OEnc;
typedef struct H264ODec H264ODec;

/* encoder: mirrors init_encoder / force_key_frame / encode_frame_yuv_i420 (openh264_wrapper.cpp) */
H264OEnc *h264o_enc_create(int w, int h, int bitrate);
void h264o_enc_destroy(H264OEnc *e);
void h264o_enc_force_idr(H264OEnc *e);
int h264o_enc_encode(H264OEnc *e, const uint8_t *i420, uint8_t *out, int cap); /* bytes, 0 = fail */
void h264o_enc_recon(const H264OEnc *e, uint8_t *i420_out);   /* deblocked recon, tight I420 */
void h264o_enc_mbinfo(const H264OEnc *e, int32_t *out);       /* 8 x int32 per MB */
int h264o_enc_last_qp(const H264OEnc *e);
/* frame skipping is on by default, as in the wrapper's OpenH264 configuration;
 * a skipped frame encodes to 0 bytes */
void h264o_enc_set_frame_skip(H264OEnc *e, int enable);
int h264o_enc_frames_skipped(const H264OEnc *e);
/* motion-search stage counters since creation: cross searches run, cross searches that moved the
 * vector, start points won by a neighbour candidate (A, B or C) */
/* {cross searches, cross searches that moved, neighbour start points won, P_Skip judges run, double-check skips,
 * intra MBs in P slices} */
void h264o_enc_me_stats(const H264OEnc *e, int32_t out[6]);
/* Decision-branch audit: the encoder's forward decisions as named classes, one per outcome.
 * h264o_enc_branch_classes: how many; h264o_enc_branch_name(c): class c's name (NULL outside the table);
 * h264o_enc_branch_counts: how often each was taken since creation (one int64 per class);
 * h264o_enc_mb_branches: beside h264o_enc_mbinfo, per MB of the last coded frame the classes it took, as
 * h264o_enc_branch_words() uint64 (bit c & 63 of word c >> 6); a row's QP classes stand in its first MB's record.
 * Counting reads decisions and makes none: no output byte depends on it. */
int h264o_enc_branch_classes(void);
const char *h264o_enc_branch_name(int c);
int h264o_enc_branch_words(void);
void h264o_enc_branch_counts(const H264OEnc *e, int64_t *out);
void h264o_enc_mb_branches(const H264OEnc *e, uint64_t *out);
/* WelsCalculateSingleCtr4x4 (h264.wasm func 1011) over 16 levels in scan order */
int h264o_single_ctr(const int16_t lv[16]);
/* PredictSadSkip (h264.wasm func 331) over the neighbour cache {top-left, top, top-right, left}: reference index (-2
 * outside, -1 intra, 0 inter), skipped flag, skip SAD */
int h264o_predict_sad_skip(const int32_t ref[4], const int32_t sk[4], const int32_t sad[4]);
/* {mv min, mv max low bits, max level, luma single-ctr max, chroma single-ctr max} */
void h264o_pskip_constants(int32_t out[5]);
int h264o_rc_row_delta(int64_t row_bits, int64_t mean);
int h264o_rc_init_qp(int w, int h, int bitrate);
int h264o_rc_idr_params(int w, int h, int bitrate, int *rmin, int *rmax);  /* first IDR QP, IDR QP range */
void h264o_rc_constants(int32_t out[8]);  /* fps, QP min/max, frame window lower/upper, IDR window, IDR ratio, skip ratio */
int h264o_table(const char *name, double *out);  /* the oracle's copy of an OpenH264 table (entry count, -1 unknown) */
/* OpenH264's rate control restated from h264.wasm */
float h264o_logf(float x);                 /* musl logf (func 483) */
int h264o_rc_qstep2qp(int32_t qstep);      /* RcConvertQStep2Qp */
int h264o_enc_gom_state(const H264OEnc *e, int32_t *out, int cap);
/* intra mode decision pieces, for tests: AnalysisVaaInfoIntra of a 16x16 source block, the
 * Intra4x4 choice of one block from its nine mode costs and availability index, the pinned constants */
int h264o_vaa_intra_var(const uint8_t *src, int stride);
int h264o_i4_choose(const int32_t c[9], int avail_index, int32_t *cost);
void h264o_md_constants(int32_t out[3]);
void h264o_enc_set_gom_exact(H264OEnc *e, int enable);  /* MB QPs by OpenH264's GOM rule (funcs 1215 / 1206) */
void h264o_enc_rc_state(const H264OEnc *e, int32_t out[16]);
size_t h264o_write_sps(int w, int h, int bitrate, uint8_t *out);
int h264o_level_idc(int w, int h, int bitrate, int *cs3);
size_t h264o_write_pps(uint8_t *out);

/* decoder: mirrors init_decoder / decode_frame_yuv_i420 */
H264ODec *h264o_dec_create(void);
void h264o_dec_destroy(H264ODec *d);
/* picture output into out_i420 (tight, cropped) -> 1: picture decoded, 2: damaged access unit concealed by a copy of the last picture (frame-copy
 * error concealment), 0: no picture, -1: error with nothing to conceal */
int h264o_dec_decode(H264ODec *d, const uint8_t *data, int size, uint8_t *out_i420, int *w, int *h);
void h264o_dec_mbinfo(const H264ODec *d, int32_t *out);
void h264o_dec_nnz(const H264ODec *d, uint8_t *out);  /* 24 TotalCoeff bytes per MB of the last picture */

/* Loop-filter test hooks (tests/dbkref.py): everything clause 8.7 reads, as the decoder holds it when it
 * calls its own filter. They change nothing of what the decoder decodes.
 * h264o_dec_set_capture(d, 1): from the next picture on, keep a copy of the picture as it stands immediately
 *   before the loop filter. h264o_dec_prefilter copies it to out as tight I420 at *coded* size (the filter's
 *   taps cross the crop line; h264o_dec_coded_size gives cw, ch) and returns its byte count cw * ch * 3 / 2,
 *   -1 when no picture was captured.
 * h264o_dec_records: H264O_REC_INTS int32 for every macroblock of the last picture, in raster order; returns
 *   the macroblock count (-1: no picture geometry yet). Layout of one record:
 *     [0]      mb type (MBT_*: 0 I_NxN, 1 I_16x16, 2 P_L0_16x16, 3 P_Skip, 4 P_16x8, 5 P_8x16, 6 P_8x8, 7 I_PCM)
 *     [1]      QPY as parsed (an I_PCM macroblock holds the running QPY; 8.7.2.2's "QPY 0" rule is the reader's)
 *     [2..17]  TotalCoeff of the 16 luma 4x4 blocks, raster order (I_PCM: 16 each)
 *     [18..21] ref_idx_l0 of the four 8x8 quadrants (-1: intra)
 *     [22..53] mv of the 16 luma 4x4 blocks, raster order, x then y, quarter samples
 *     [54]     first_mb_in_slice of the macroblock's slice
 *     [55]     disable_deblocking_filter_idc   [56] FilterOffsetA   [57] FilterOffsetB  (of that slice)
 *     [58]     chroma_qp_index_offset of the picture's PPS   [59] 0 (reserved) */
#define H264O_REC_INTS 60
void h264o_dec_set_capture(H264ODec *d, int on);
int h264o_dec_coded_size(const H264ODec *d, int *cw, int *ch);
int h264o_dec_prefilter(const H264ODec *d, uint8_t *out);
int h264o_dec_records(const H264ODec *d, int32_t *out);

/* Reconstruction test hook (tests/reconref.py): the parsed syntax of every macroblock of the last picture, before
 * any derivation -- what clauses 8.3, 8.4 and 8.5 start from. Kept only while h264o_dec_set_capture is on; it changes
 * nothing of what the decoder decodes. Returns the macroblock count (-1: nothing captured). The entries are cleared when
 * a picture opens, so a macroblock the picture's slices did not cover reads all zero, and they are released by the first
 * picture decoded with the capture off (-1 from then on). H264O_SYN_INTS int32 per macroblock, raster order:
 *     [0]        mb_type as parsed: the ue(v) value, in a P slice 0..4 inter and 5..30 intra (Table 7-13 after the
 *                offset of 5); -1 for a macroblock of an mb_skip_run
 *     [1]        slice_type % 5 of its slice (0 P, 2 I)
 *     [2..5]     sub_mb_type of the four sub-macroblocks (P_8x8)
 *     [6..37]    mvd_l0 of every partition / sub-macroblock partition in parse order, x then y
 *     [38..53]   prev_intra4x4_pred_mode_flag by luma4x4BlkIdx   [54..69] rem_intra4x4_pred_mode by luma4x4BlkIdx
 *     [70]       intra_chroma_pred_mode   [71] coded_block_pattern as mapped from [76], its codeNum (both 0 for
 *                I_16x16, whose pattern is part of mb_type)   [72] mb_qp_delta (0 when absent)
 *     [73]       SliceQPY   [74] first_mb_in_slice   [75] chroma_qp_index_offset of the PPS
 *     [77]       disable_deblocking_filter_idc   [78] FilterOffsetA   [79] FilterOffsetB  (of the slice)
 *     [80..95]   Intra16x16DCLevel, scan order
 *     [96..351]  the 16 luma blocks by luma4x4BlkIdx, 16 ints each: Luma4x4 levels in scan order, or for I_16x16
 *                the 15 Intra16x16ACLevel in entries 0..14
 *     [352..359] chroma DC levels, Cb then Cr, 4 each in parse order
 *     [360..487] chroma AC levels, Cb then Cr, 4 blocks of 16 ints each: the 15 levels in entries 0..14
 *     [488..871] the 384 pcm_sample values (luma, Cb, Cr) */
#define H264O_SYN_INTS 872
int h264o_dec_syntax(const H264ODec *d, int32_t *out);

/* test-stream helpers (tests/streamgen.py): CAVLC bits of one residual block (0/1 per byte; returns
 * the bit count, -1 if cap is too small) and the coded_block_pattern codeNum of cbp (Table 9-4) */
int h264o_cavlc_bits(const int16_t *coef, int maxnum, int nc, uint8_t *bits, int cap);
int h264o_cbp_code(int cbp, int intra);

/* wrapper colour conversion: rgba_to_yuv (openh264_wrapper.cpp:22-40),
 * yuv_to_rgba_optimized (:150-195) */
void h264o_rgba_to_i420(const uint8_t *rgba, int w, int h, uint8_t *i420_out);
void h264o_i420_to_rgba(const uint8_t *y, const uint8_t *u, const uint8_t *v, int w, int h, int ys, int uvs,
                        uint8_t *rgba_out);

#ifdef __cplusplus
}
#endif
#endif
