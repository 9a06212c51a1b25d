// enc_input.inc -- the encoder's input chain (EncInput, runtime_enc.inc; DESIGN.md §5.16): the stages that work on the
// input area in front of the frame step, in one place: the order they run in, the first-frame transition of each, the
// setters that allocate and free their device state, and the release. capi_enc.inc forwards to this file.
namespace h264mi {

// ---------------------------------------------------------------- a stage's device state
// free: the stream has finished with the state, or never saw it
template <class T> static void state_free(T *&p) { (void)hipFree(p); p = nullptr; }
// drop: the stream may still work on the state -- what is there is freed after the stream has finished with it
template <class... T> static void state_drop(EncCtx *c, T *&...p) {
    if (!(... || p)) return;
    (void)hipStreamSynchronize(c->stream);
    (state_free(p), ...);
}
// ensure: allocated when absent. 0: it was there, 1: it is fresh -- the caller resets has --, -1: no memory
template <class T> static int state_ensure(T *&p, size_t bytes) {
    if (p) return 0;
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return -1; }
    return 1;
}
// enc_free's part. Nothing waits here: h264mi_enc_destroy has synchronised the stream, the wrapper's encoder has no stage
static void enc_input_release(EncCtx *c) {
    state_free(c->in.di.d_prev); state_free(c->in.dn.d_prev); state_free(c->in.lv.d_mem); state_free(c->in.sp.d_buf); state_free(c->in.sc.d_words);
    state_free(c->in.sc.d_thumb);
}

// ---------------------------------------------------------------- the chain
// the tail of every entry point that codes the input area: the deinterlacer in force (DESIGN.md §5.15;
// deinterlace.hip; nothing when off) -- in place against the previous unfiltered frames, which the same launch
// replaces; the first frame spatial only --, the pre-filter in force (DESIGN.md §5.13; denoise.hip;
// nothing when off) -- the first frame only copied to the state, every later one filtered in place against the state,
// which receives the same bytes --, the levels stage in force (DESIGN.md §5.19; levels.hip; nothing when off) -- in place
// on the input area: AUTO the histogram, the decision, which advances the stream's ends, and the tables' application,
// FIXED the application of the tables the setter wrote; the two states in front of it never hold a levelled frame --,
// the spatial filter in force (DESIGN.md §5.18; spatial.hip; nothing when off) -- out
// of place into the stage's own frames, which are the current frames `cur` of everything behind it, so the denoiser's
// state never holds a sharpened frame --, the privacy masks in force (the same unit; nothing without a list) in place
// on the current frames, the key-frame policy in force (below), the overlay list in force blended into them
// (DESIGN.md §5.6; overlay.hip; nothing without a list), then the frame step on them. A launch that fails ends the
// call with -1 where it stands: no frame is submitted, and the states of the steps in front of it have advanced
static int enc_code_input(EncCtx *c) {
    EncInput &in = c->in;
    uint8_t *cur = c->d_src;  // the current frames: the input area, behind the spatial filter its buffer
    if (in.di.on) {
        if (launch_deinterlace_i420(c->d_src, in.di.d_prev, c->d_src, in.di.has ? in.di.d_prev : nullptr, c->w, c->h, c->S, in.di.p, nullptr, c->stream) != 0)
            return -1;
        in.di.has = true;
    }
    if (in.dn.on) {
        if (!in.dn.has) {
            if (hipMemcpyAsync(in.dn.d_prev, c->d_src, (size_t)c->S * c->fbytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
            in.dn.has = true;
        } else if (launch_denoise_i420(c->d_src, in.dn.d_prev, c->d_src, in.dn.d_prev, c->w, c->h, c->S, in.dn.p, nullptr, c->stream) != 0) {
            return -1;
        }
    }
    if (in.lv.on) {
        EncInput::Levels &l = in.lv;
        if (l.p.mode == H264MI_LEVELS_AUTO) {
            if (launch_hist_i420(l.hist(), c->d_src, c->w, c->h, c->S, c->stream) != 0 ||
                launch_levels_decide(l.luts(c->S), l.hist(), l.state(c->S), l.record(c->S), c->w, c->h, c->S, l.p, c->stream) != 0)
                return -1;
        }
        if (launch_lut_i420(c->d_src, c->d_src, c->w, c->h, c->S, l.luts(c->S), 1, c->stream) != 0) return -1;
    }
    if (in.sp.on) {
        if (launch_spatial_i420(in.sp.d_buf, cur, c->w, c->h, c->S, in.sp.p, c->stream) != 0) return -1;
        cur = in.sp.d_buf;
    }
    if (!in.pv.list.empty() && launch_privacy_i420(cur, c->w, c->h, in.pv.list.data(), (int)in.pv.list.size(), c->stream) != 0) return -1;
    // the key-frame policy in force (DESIGN.md §5.14; scenecut.hip; nothing when off): the detector -- the first frame
    // only stores its thumbnails, every later one advances them in place and leaves its statistics; no launch with
    // share == 0 --, then the decision, which sets EncState::force_idr in front of the frame step's begin kernel
    if (in.sc.on) {
        uint32_t *stats = nullptr;
        if (in.sc.p.share > 0) {
            const bool has = in.sc.has;
            if (has) stats = in.sc.d_words + 16 * (size_t)c->S;
            if (launch_scenecut_i420(stats, in.sc.d_thumb, cur, has ? in.sc.d_thumb : nullptr, c->w, c->h, c->S, in.sc.p, c->stream) != 0)
                return -1;
            in.sc.has = true;
        }
        if (launch_scenecut_decide(c->d_st, in.sc.d_words, stats, c->S, in.sc.p, c->stream) != 0) return -1;
    }
    if (!in.ov.list.empty() &&
        launch_overlay_i420(cur, c->w, c->h, in.ov.sprites, in.ov.w, in.ov.h, in.ov.list.data(), (int)in.ov.list.size(), c->stream) != 0)
        return -1;
    return enc_frame(c, cur);
}
// h264mi_enc_encode: with every stage off the caller's frames are coded where they lie; with the deinterlacer, the
// pre-filter, the levels stage, the spatial filter or the key-frame policy on or a mask or overlay list in force they are copied into the input area, filtered,
// looked at and blended there and coded from there
static int enc_encode(EncCtx *c, const void *d_frames) {
    if (!c->in.any()) return enc_frame(c, (const uint8_t *)d_frames);
    if (d_frames != (const void *)c->d_src) {
        const size_t nb = (size_t)c->S * c->fbytes;
        if (byte_ranges_overlap(d_frames, nb, c->d_src, nb)) return -1;  // partly inside the input area
        if (hipMemcpyAsync(c->d_src, d_frames, nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
    }
    return enc_code_input(c);
}
// The entry points that resample on the way into the input area (scaled, oriented, composed) are refused while the
// deinterlacer is on: it belongs in front of a vertical resampling, which mixes the lines of the two fields, and in
// the chain it runs behind what these entry points write
static bool enc_resampling_refused(const EncCtx *c) { return c->in.di.on; }

// ---------------------------------------------------------------- the setters
// A refused call leaves the setting in force. What a getter answers: 1 and the parameters in force, 0 when off
template <class Stage, class P> static int stage_get(const Stage &s, P *out) {
    if (s.on && out) *out = s.p;
    return s.on ? 1 : 0;
}
// the two stages whose state is the S previous frames; p has passed the stage's own check. off: the state goes
template <class Stage, class P> static int set_prev_frame_stage(EncCtx *c, Stage &s, const P *p, bool off) {
    if (off) { state_drop(c, s.d_prev); s.on = s.has = false; return 0; }
    if (!canvas_ok(c->w, c->h)) return -1;
    const int fresh = state_ensure(s.d_prev, (size_t)c->S * c->fbytes);
    if (fresh < 0) return -1;
    if (fresh) s.has = false;
    s.p = *p; s.on = true;
    return 0;
}
// the pre-filter: NULL or both strengths 0 turn it off
static int enc_set_denoise(EncCtx *c, const h264mi_denoise *p) {
    if (p && !denoise_ok(p)) return -1;
    return set_prev_frame_stage(c, c->in.dn, p, !p || (p->strength_y == 0 && p->strength_c == 0));
}
// the deinterlacer: only NULL turns it off
static int enc_set_deinterlace(EncCtx *c, const h264mi_deinterlace *p) {
    if (p && !deinterlace_ok(p)) return -1;
    return set_prev_frame_stage(c, c->in.di, p, !p);
}
// the levels stage: NULL or an inert setting turn it off and free its words. They are allocated, and the state and the
// record zeroed on the stream, when it is turned on; a change of the parameters keeps them. FIXED: the tables and the
// record come from the parameters alone and are written here, once, in stream order behind the frames submitted so far
static int enc_set_levels(EncCtx *c, const h264mi_levels *p) {
    if (p && !levels_ok(p)) return -1;
    EncInput::Levels &l = c->in.lv;
    if (!p || levels_inert(*p)) { state_drop(c, l.d_mem); l.on = false; return 0; }
    if (!canvas_ok(c->w, c->h)) return -1;
    const int fresh = state_ensure(l.d_mem, EncInput::Levels::bytes(c->S));
    if (fresh < 0) return -1;
    if ((fresh && hipMemsetAsync(l.state(c->S), 0, 48 * (size_t)c->S, c->stream) != hipSuccess) ||
        (p->mode == H264MI_LEVELS_FIXED &&
         launch_levels_decide(l.luts(c->S), nullptr, nullptr, l.record(c->S), c->w, c->h, c->S, *p, c->stream) != 0)) {
        if (fresh) { state_drop(c, l.d_mem); l.on = false; }  // an earlier setting's words stay, and stay in force
        return -1;
    }
    l.p = *p; l.on = true;
    return 0;
}
// the spatial filter: NULL or an inert setting turn it off and free the frames it filtered into
static int enc_set_spatial(EncCtx *c, const h264mi_spatial *p) {
    if (p && !spatial_ok(p)) return -1;
    EncInput::Spatial &s = c->in.sp;
    if (!p || spatial_inert(*p)) { state_drop(c, s.d_buf); s.on = false; return 0; }
    if (!canvas_ok(c->w, c->h) || state_ensure(s.d_buf, (size_t)c->S * c->fbytes) < 0) return -1;
    s.p = *p; s.on = true;
    return 0;
}
// the privacy masks: n == 0 clears the list. The entries are copied; frame is the stream
static int enc_set_privacy(EncCtx *c, const h264mi_privacy *list, int n) {
    if (n == 0) { c->in.pv.list.clear(); return 0; }
    if (!privacy_ok(list, n, c->w, c->h, c->S)) return -1;
    c->in.pv.list.assign(list, list + n);
    return 0;
}
// the key-frame policy: NULL or share == 0 && max_gap == 0 turn it off. The words are zeroed on the stream when they
// are allocated and kept across a change of the parameters; the thumbnails exist only with share > 0
static int enc_set_scenecut(EncCtx *c, const h264mi_scenecut *p) {
    if (p && !scenecut_ok(p)) return -1;
    EncInput::Scenecut &s = c->in.sc;
    if (!p || (p->share == 0 && p->max_gap == 0)) { state_drop(c, s.d_words, s.d_thumb); s.on = s.has = false; return 0; }
    if (!canvas_ok(c->w, c->h)) return -1;
    const size_t wbytes = 24 * sizeof(uint32_t) * (size_t)c->S;
    const int fresh_words = state_ensure(s.d_words, wbytes);
    if (fresh_words < 0) return -1;
    if (fresh_words && hipMemsetAsync(s.d_words, 0, wbytes, c->stream) != hipSuccess) { state_free(s.d_words); return -1; }
    const bool had_thumb = s.d_thumb != nullptr;
    if (p->share == 0) {
        state_drop(c, s.d_thumb);  // period only: no detector runs, the thumbnails of an earlier setting go
    } else if (state_ensure(s.d_thumb, (size_t)c->S * thumb_bytes(c->w, c->h)) < 0) {
        if (fresh_words) state_drop(c, s.d_words);  // the zeroing is on the stream; words of an earlier setting stay
        return -1;
    }
    if (!had_thumb || !s.d_thumb) s.has = false;
    s.p = *p; s.on = true;
    return 0;
}
// the overlay list: nov == 0 clears it. The placements are copied, the sprites stay the caller's
static int enc_set_overlays(EncCtx *c, const void *d_sprites, int ow, int oh, int nsprites, const h264mi_overlay *ov, int nov) {
    EncInput::Overlays &o = c->in.ov;
    if (nov == 0) { o.list.clear(); o.sprites = nullptr; return 0; }
    if (!d_sprites || !overlay_args_ok(c->w, c->h, c->S, ow, oh, nsprites, ov, nov) ||
        byte_ranges_overlap(c->d_src, c->S * i420_bytes(c->w, c->h), d_sprites, nsprites * i420a_bytes(ow, oh)))
        return -1;
    o.list.assign(ov, ov + nov);
    o.sprites = (const uint8_t *)d_sprites; o.w = ow; o.h = oh;
    return 0;
}

}  // namespace h264mi
