"""ctypes wrapper of the CPU oracle (oracle/h264o_api.h) -- TEST INFRASTRUCTURE ONLY."""
import ctypes
import numpy as np

vp = ctypes.c_void_p


class Oracle:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.h264o_enc_create.restype = vp
        L.h264o_enc_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.h264o_enc_destroy.argtypes = [vp]
        L.h264o_enc_force_idr.argtypes = [vp]
        L.h264o_enc_encode.argtypes = [vp, vp, vp, ctypes.c_int]
        L.h264o_enc_recon.argtypes = [vp, vp]
        L.h264o_enc_mbinfo.argtypes = [vp, vp]
        L.h264o_enc_last_qp.argtypes = [vp]
        L.h264o_enc_set_frame_skip.argtypes = [vp, ctypes.c_int]
        L.h264o_enc_frames_skipped.argtypes = [vp]
        L.h264o_enc_me_stats.argtypes = [vp, vp]
        L.h264o_enc_branch_name.restype = ctypes.c_char_p
        L.h264o_enc_branch_name.argtypes = [ctypes.c_int]
        L.h264o_enc_branch_counts.argtypes = [vp, vp]
        L.h264o_enc_mb_branches.argtypes = [vp, vp]
        L.h264o_rc_init_qp.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.h264o_rc_qstep2qp.argtypes = [ctypes.c_int32]
        L.h264o_logf.argtypes = [ctypes.c_float]
        L.h264o_logf.restype = ctypes.c_float
        L.h264o_enc_set_gom_exact.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.h264o_enc_rc_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.h264o_enc_gom_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.h264o_write_sps.restype = ctypes.c_size_t
        L.h264o_write_sps.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
        L.h264o_write_pps.restype = ctypes.c_size_t
        L.h264o_write_pps.argtypes = [vp]
        L.h264o_dec_create.restype = vp
        L.h264o_dec_destroy.argtypes = [vp]
        L.h264o_dec_decode.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        L.h264o_dec_mbinfo.argtypes = [vp, vp]
        L.h264o_dec_set_capture.argtypes = [vp, ctypes.c_int]
        L.h264o_dec_coded_size.argtypes = [vp, vp, vp]
        L.h264o_dec_prefilter.argtypes = [vp, vp]
        L.h264o_dec_records.argtypes = [vp, vp]
        L.h264o_dec_syntax.argtypes = [vp, vp]
        L.h264o_table.argtypes = [ctypes.c_char_p, vp]
        L.h264o_rgba_to_i420.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.h264o_i420_to_rgba.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
        self.L = L

    def encoder(self, w, h, br):
        return OEnc(self.L, w, h, br)

    def branch_names(self):
        """the encoder's decision-branch classes, in table order (h264o_enc_branch_name)"""
        return [self.L.h264o_enc_branch_name(c).decode() for c in range(self.L.h264o_enc_branch_classes())]

    def decoder(self):
        return ODec(self.L)

    def rgba_to_i420(self, rgba, w, h):
        out = np.zeros(w * h * 3 // 2, np.uint8)
        rgba = np.ascontiguousarray(rgba, np.uint8)
        self.L.h264o_rgba_to_i420(rgba.ctypes.data, w, h, out.ctypes.data)
        return out

    def i420_to_rgba(self, i420, w, h):
        i420 = np.ascontiguousarray(i420, np.uint8)
        out = np.zeros(w * h * 4, np.uint8)
        y = i420.ctypes.data
        self.L.h264o_i420_to_rgba(y, y + w * h, y + w * h + (w // 2) * (h // 2), w, h, w, w // 2, out.ctypes.data)
        return out


class OEnc:
    def __init__(self, L, w, h, br):
        self.L, self.w, self.h = L, w, h
        self.e = vp(L.h264o_enc_create(w, h, br))
        assert self.e.value
        self.buf = np.zeros(w * h * 4 + 65536, np.uint8)

    def encode(self, i420):
        i420 = np.ascontiguousarray(i420, np.uint8)
        n = self.L.h264o_enc_encode(self.e, i420.ctypes.data, self.buf.ctypes.data, self.buf.size)
        return self.buf[:n].tobytes()

    def force_idr(self):
        self.L.h264o_enc_force_idr(self.e)

    def set_frame_skip(self, on):
        self.L.h264o_enc_set_frame_skip(self.e, 1 if on else 0)

    def set_gom_exact(self, on):
        self.L.h264o_enc_set_gom_exact(self.e, 1 if on else 0)

    RC_FIELDS = ('skipped', 'qp', 'avg_qp', 'target', 'remaining', 'fullness', 'continual', 'cmplx', 'min_qp',
                 'max_qp', 'bpf', 'pframes', 'idrs', 'skip_flag', 'remaining_weights', 'coded_in_vgop')

    def rc_state(self):
        """the rate control's state after the last encode call (oracle h264o_enc_rc_state)"""
        out = (ctypes.c_int32 * 16)()
        self.L.h264o_enc_rc_state(self.e, out)
        return dict(zip(self.RC_FIELDS, list(out)))

    def gom_state(self):
        """exact GOM mode: the last P frame's per-GOM [QP, slice bits before it, target bits, last coded MB + 1]"""
        G = self.L.h264o_enc_gom_state(self.e, None, 0)
        out = (ctypes.c_int32 * (4 * max(G, 1)))()
        self.L.h264o_enc_gom_state(self.e, out, 4 * G)
        return [list(out[4 * g:4 * g + 4]) for g in range(G)]

    def branch_counts(self):
        """how often each decision-branch class was taken since creation (h264o_enc_branch_counts)"""
        out = np.zeros(self.L.h264o_enc_branch_classes(), np.int64)
        self.L.h264o_enc_branch_counts(self.e, out.ctypes.data)
        return out

    def mb_branches(self):
        """per MB of the last coded frame, the indices of the classes it took (h264o_enc_mb_branches)"""
        nw, nmb = self.L.h264o_enc_branch_words(), ((self.w + 15) // 16) * ((self.h + 15) // 16)
        out = np.zeros(nmb * nw, np.uint64)
        self.L.h264o_enc_mb_branches(self.e, out.ctypes.data)
        bits = np.unpackbits(out.view(np.uint8).reshape(nmb, nw * 8), axis=1, bitorder='little')
        return [np.flatnonzero(r).tolist() for r in bits]

    def mbinfo(self):
        """int32 [MBs, 8] of the last coded frame: type, QP, cbp, mvx, mvy, I16 mode, chroma mode, TotalCoeff sum"""
        out = np.zeros(((self.w + 15) // 16) * ((self.h + 15) // 16) * 8, np.int32)
        self.L.h264o_enc_mbinfo(self.e, out.ctypes.data)
        return out.reshape(-1, 8)

    def recon(self):
        out = np.zeros(self.w * self.h * 3 // 2, np.uint8)
        self.L.h264o_enc_recon(self.e, out.ctypes.data)
        return out

    def last_qp(self):
        return self.L.h264o_enc_last_qp(self.e)

    def __del__(self):
        try:
            self.L.h264o_enc_destroy(self.e)
        except Exception:
            pass


class ODec:
    def __init__(self, L):
        self.L = L
        self.d = vp(L.h264o_dec_create())
        self.out = np.zeros(4096 * 2304 * 3 // 2, np.uint8)

    def decode(self, nal):
        """-> (rc, tight I420 bytes or None, w, h)"""
        a = np.frombuffer(nal, np.uint8).copy() if len(nal) else np.zeros(1, np.uint8)
        w, h = ctypes.c_int(0), ctypes.c_int(0)
        rc = self.L.h264o_dec_decode(self.d, a.ctypes.data, len(nal), self.out.ctypes.data, ctypes.byref(w), ctypes.byref(h))
        if rc in (1, 2):  # 2: damaged access unit concealed by a copy of the last picture
            return rc, self.out[:w.value * h.value * 3 // 2].copy(), w.value, h.value
        return rc, None, w.value, h.value

    REC_INTS = 60  # H264O_REC_INTS

    def set_capture(self, on=True):
        """keep each picture as it stands before the loop filter (h264o_dec_set_capture)"""
        self.L.h264o_dec_set_capture(self.d, 1 if on else 0)

    def coded_size(self):
        cw, ch = ctypes.c_int(0), ctypes.c_int(0)
        assert self.L.h264o_dec_coded_size(self.d, ctypes.byref(cw), ctypes.byref(ch)) == 0
        return cw.value, ch.value

    def prefilter(self):
        """-> (Y, U, V) of the last picture before its loop filter, at coded size"""
        cw, ch = self.coded_size()
        buf = np.zeros(cw * ch * 3 // 2, np.uint8)
        assert self.L.h264o_dec_prefilter(self.d, buf.ctypes.data) == buf.size
        n = cw * ch
        return (buf[:n].reshape(ch, cw), buf[n:n + n // 4].reshape(ch // 2, cw // 2),
                buf[n + n // 4:].reshape(ch // 2, cw // 2))

    def records(self):
        """-> int32 [macroblocks, REC_INTS]: what clause 8.7 reads of every macroblock (layout: h264o_api.h)"""
        cw, ch = self.coded_size()
        out = np.zeros((cw // 16) * (ch // 16) * self.REC_INTS, np.int32)
        assert self.L.h264o_dec_records(self.d, out.ctypes.data) == out.size // self.REC_INTS
        return out.reshape(-1, self.REC_INTS)

    SYN_INTS = 872  # H264O_SYN_INTS

    def syntax(self):
        """-> int32 [macroblocks, SYN_INTS]: the parsed syntax elements of every macroblock (layout: h264o_api.h)"""
        cw, ch = self.coded_size()
        out = np.zeros((cw // 16) * (ch // 16) * self.SYN_INTS, np.int32)
        assert self.L.h264o_dec_syntax(self.d, out.ctypes.data) == out.size // self.SYN_INTS
        return out.reshape(-1, self.SYN_INTS)

    def __del__(self):
        try:
            self.L.h264o_dec_destroy(self.d)
        except Exception:
            pass
