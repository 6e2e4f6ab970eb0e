"""ctypes binding of include/ractip_hot.h (the C ABI of libractip_hot.so).

Thin by design: every method is one C call.  There is NO fallback: if the HIP
library is missing or no GPU is present, creation raises.
"""
import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RACTIP_HOT_LIB") or os.path.join(PKG, "libractip_hot.so")   # override: tuning builds (tools/build_variant.py)

RH_MODEL_CONTRAFOLD = 0
RH_MODEL_VIENNA_BL = 1
RH_MODE_INHERIT, RH_MODE_AUTO, RH_MODE_LOG, RH_MODE_LINEAR = -1, 0, 1, 2

EXPORTS = [
    "rh_create", "rh_destroy", "rh_last_error", "rh_set_mode", "rh_last_path", "rh_bpp", "rh_unpaired", "rh_fold", "rh_duplex",
    "rh_batch_upload", "rh_batch_compute", "rh_batch_results", "rh_batch_candidates",
    "rh_batch_timings", "rh_batch_device_views", "rh_batch_logz", "rh_batch_candidates_all", "rh_batch_layout",
    "rh_batch_results_all", "rh_set_max_w", "rh_get_max_w", "rh_set_overlap", "rh_batch_kernels", "rh_set_hybrid", "rh_last_hybrid_path", "rh_fold_constrained", "rh_cofold_constrained",
    "rh_host_alloc", "rh_host_free", "rh_batch_fallbacks", "rh_create_vienna", "rh_vienna_semantics", "rh_set_scale_memory", "rh_set_kernel_timing", "rh_kernel_times",
    "rh_set_duplex_mode", "rh_get_duplex_mode",
    "rh_batch_upload_constrained", "rh_debug_batch_allow_mask",
    "rh_batch_upload_indexed", "rh_batch_index", "rh_batch_candidates_seq_all", "rh_batch_upload_indexed_constrained",
    "rh_batch_packed_layout", "rh_batch_results_packed_f32", "rh_batch_pack_time",
    "rh_set_region_accessibility", "rh_get_region_accessibility", "rh_batch_acc_time",
    "rh_local_fold", "rh_local_layout", "rh_local_results", "rh_local_candidates", "rh_set_local_chunk", "rh_local_times",
    "rh_local_duplex", "rh_local_hp_layout", "rh_local_hp_results",
    "rh_local_duplex2", "rh_local_hp2_layout", "rh_local_hp2_results", "rh_local_hp2_candidates", "rh_set_local_tile", "rh_local_hp2_tile",
    "rh_local_hp2_times",
    "rh_span_fold", "rh_span_times", "rh_span_fold_acc", "rh_span_acc_times",
    "rh_span_fold_batch", "rh_span_batch_layout", "rh_span_batch_item", "rh_span_batch_results", "rh_span_batch_candidates",
    "rh_set_span_batch_bytes", "rh_span_batch_times",
    "rh_span_fold_constrained", "rh_span_fold_batch_constrained",
    "rh_set_span_contrafold", "rh_get_span_contrafold",
    "rh_debug_vienna_cell", "rh_debug_vienna_value",   # loader inspection (host only; used by the CPU tests of the loader)
]


class RhError(RuntimeError):
    pass


class Cand(ctypes.Structure):
    _fields_ = [("i", ctypes.c_int), ("j", ctypes.c_int), ("p", ctypes.c_float)]


_lib = None


def load_library():
    """dlopen libractip_hot.so and declare the prototypes (no GPU needed for this)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RhError("%s is missing: run `python -m ractip_amd.build` (or __graft_entry__.build()) first; "
                      "there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, cp, ci, dp = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    L.rh_create.restype = vp
    L.rh_create_vienna.restype = vp
    L.rh_create_vienna.argtypes = [ci, cp, ci, cp, ci]
    L.rh_vienna_semantics.argtypes = [vp]
    L.rh_create.argtypes = [ci, ci, cp]
    L.rh_destroy.restype = None
    L.rh_destroy.argtypes = [vp]
    L.rh_last_error.restype = cp
    L.rh_last_error.argtypes = [vp]
    L.rh_set_mode.argtypes = [vp, ci]
    L.rh_set_mode.restype = ci
    L.rh_set_duplex_mode.argtypes = [vp, ci]
    L.rh_set_duplex_mode.restype = ci
    L.rh_get_duplex_mode.argtypes = [vp]
    L.rh_get_duplex_mode.restype = ci
    L.rh_last_path.argtypes = [vp]
    L.rh_set_overlap.argtypes = [vp, ci]
    L.rh_set_scale_memory.argtypes = [vp, ci]
    L.rh_set_kernel_timing.argtypes = [vp, ci]
    L.rh_set_kernel_timing.restype = ci
    L.rh_kernel_times.argtypes = [vp, vp, vp]
    L.rh_kernel_times.restype = ci
    L.rh_set_scale_memory.restype = ci
    L.rh_last_hybrid_path.argtypes = [vp]
    L.rh_last_hybrid_path.restype = ci
    L.rh_set_hybrid.argtypes = [vp, ci]
    L.rh_set_hybrid.restype = ci
    L.rh_batch_kernels.argtypes = [vp, vp, vp, vp]
    L.rh_batch_kernels.restype = ci
    L.rh_set_overlap.restype = ci
    L.rh_set_max_w.argtypes = [vp, ci]
    L.rh_set_max_w.restype = ci
    L.rh_get_max_w.argtypes = [vp]
    L.rh_get_max_w.restype = ci
    L.rh_last_path.restype = ci
    L.rh_bpp.argtypes = [vp, cp, ci, cp, vp, vp]
    L.rh_unpaired.argtypes = [vp, cp, ci, ci, vp]
    L.rh_fold.argtypes = [vp, cp, ci, vp, vp, vp]
    L.rh_fold_constrained.argtypes = [vp, cp, ci, cp, vp, vp, vp]
    L.rh_fold_constrained.restype = ci
    L.rh_cofold_constrained.argtypes = [vp, cp, ci, cp, ci, cp, vp, vp]
    L.rh_cofold_constrained.restype = ci
    L.rh_duplex.argtypes = [vp, cp, ci, cp, ci, vp, vp]
    L.rh_batch_upload.argtypes = [vp, ci, ctypes.POINTER(cp), ctypes.POINTER(ci), ctypes.POINTER(cp), ctypes.POINTER(ci)]
    L.rh_batch_upload_constrained.argtypes = L.rh_batch_upload.argtypes + [ctypes.POINTER(cp)] * 3
    L.rh_batch_upload_constrained.restype = ci
    L.rh_batch_upload_indexed.argtypes = [vp, ci, ctypes.POINTER(cp), ctypes.POINTER(ci), ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.rh_batch_upload_indexed.restype = ci
    L.rh_batch_upload_indexed_constrained.argtypes = L.rh_batch_upload_indexed.argtypes + [ctypes.POINTER(cp)] * 3
    L.rh_batch_upload_indexed_constrained.restype = ci
    L.rh_batch_index.argtypes = [vp, vp, vp, vp, vp]
    L.rh_batch_index.restype = ci
    L.rh_batch_candidates_seq_all.argtypes = [vp, ci, ctypes.c_float, vp, ci, vp]
    L.rh_batch_candidates_seq_all.restype = ci
    L.rh_debug_batch_allow_mask.argtypes = [vp, ci, ci, vp, vp]
    L.rh_debug_batch_allow_mask.restype = ci
    L.rh_batch_compute.argtypes = [vp]
    L.rh_batch_results.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.rh_batch_candidates.argtypes = [vp, ci, ci, ctypes.c_float, vp, ci]
    L.rh_batch_candidates_all.argtypes = [vp, ci, ctypes.c_float, vp, ci, vp]
    L.rh_batch_layout.argtypes = [vp, vp, vp, vp, vp]
    L.rh_batch_results_all.argtypes = [vp, vp, vp, vp, vp]
    L.rh_batch_timings.argtypes = [vp, vp, vp]
    L.rh_batch_logz.argtypes = [vp, vp]
    L.rh_batch_device_views.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rh_batch_fallbacks.argtypes = [vp, ci, vp, ci]
    L.rh_batch_fallbacks.restype = ci
    L.rh_batch_packed_layout.argtypes = [vp, vp, vp, vp, vp]
    L.rh_batch_packed_layout.restype = ci
    L.rh_batch_results_packed_f32.argtypes = [vp, vp, vp, vp, vp]
    L.rh_batch_results_packed_f32.restype = ci
    L.rh_batch_pack_time.argtypes = [vp, vp]
    L.rh_batch_pack_time.restype = ci
    L.rh_set_region_accessibility.argtypes = [vp, ci]
    L.rh_set_region_accessibility.restype = ci
    L.rh_get_region_accessibility.argtypes = [vp]
    L.rh_get_region_accessibility.restype = ci
    L.rh_batch_acc_time.argtypes = [vp, vp]
    L.rh_batch_acc_time.restype = ci
    L.rh_local_fold.argtypes = [vp, cp, ci, ci, ci]
    L.rh_local_fold.restype = ci
    L.rh_local_layout.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rh_local_layout.restype = ci
    L.rh_local_results.argtypes = [vp, vp, vp, vp]
    L.rh_local_results.restype = ci
    L.rh_local_candidates.argtypes = [vp, ci, ctypes.c_float, vp, ci]
    L.rh_local_candidates.restype = ci
    L.rh_set_local_chunk.argtypes = [vp, ci]
    L.rh_set_local_chunk.restype = ci
    L.rh_local_times.argtypes = [vp, vp]
    L.rh_local_times.restype = ci
    L.rh_span_fold.argtypes = [vp, cp, ci, ci]
    L.rh_span_fold.restype = ci
    L.rh_span_times.argtypes = [vp, vp]
    L.rh_span_times.restype = ci
    L.rh_span_fold_acc.argtypes = [vp, cp, ci, ci, ci]
    L.rh_span_fold_acc.restype = ci
    L.rh_span_acc_times.argtypes = [vp, vp]
    L.rh_span_acc_times.restype = ci
    L.rh_span_fold_batch.argtypes = [vp, vp, vp, ci, ci, ci]
    L.rh_span_fold_batch.restype = ci
    L.rh_span_batch_layout.argtypes = [vp, vp, vp, vp]
    L.rh_span_batch_layout.restype = ci
    L.rh_span_batch_item.argtypes = [vp, ci, vp, vp, vp]
    L.rh_span_batch_item.restype = ci
    L.rh_span_batch_results.argtypes = [vp, ci, vp, vp, vp]
    L.rh_span_batch_results.restype = ci
    L.rh_span_batch_candidates.argtypes = [vp, ci, ci, ctypes.c_float, vp, ci]
    L.rh_span_batch_candidates.restype = ci
    L.rh_set_span_batch_bytes.argtypes = [vp, ctypes.c_size_t]
    L.rh_set_span_batch_bytes.restype = ci
    L.rh_span_batch_times.argtypes = [vp, vp]
    L.rh_span_batch_times.restype = ci
    L.rh_span_fold_constrained.argtypes = [vp, cp, ci, cp, ci, ci]
    L.rh_span_fold_constrained.restype = ci
    L.rh_span_fold_batch_constrained.argtypes = [vp, vp, vp, ci, vp, ci, ci]
    L.rh_span_fold_batch_constrained.restype = ci
    L.rh_set_span_contrafold.argtypes = [vp, ci]
    L.rh_set_span_contrafold.restype = ci
    L.rh_get_span_contrafold.argtypes = [vp]
    L.rh_get_span_contrafold.restype = ci
    L.rh_local_duplex.argtypes = [vp, cp, ci, cp, ci, ci, ci, ci]
    L.rh_local_duplex.restype = ci
    L.rh_local_hp_layout.argtypes = [vp, vp, vp, vp, vp]
    L.rh_local_hp_layout.restype = ci
    L.rh_local_hp_results.argtypes = [vp, vp, vp]
    L.rh_local_hp_results.restype = ci
    L.rh_local_duplex2.argtypes = [vp, cp, ci, cp, ci, ci, ci, ci, ci]
    L.rh_local_duplex2.restype = ci
    L.rh_local_hp2_layout.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.rh_local_hp2_layout.restype = ci
    L.rh_local_hp2_results.argtypes = [vp, vp, vp]
    L.rh_local_hp2_results.restype = ci
    L.rh_local_hp2_candidates.argtypes = [vp, ctypes.c_float, vp, ci]
    L.rh_local_hp2_candidates.restype = ci
    L.rh_set_local_tile.argtypes = [vp, ci, ci]
    L.rh_set_local_tile.restype = ci
    L.rh_local_hp2_tile.argtypes = [vp, vp, vp]
    L.rh_local_hp2_tile.restype = ci
    L.rh_local_hp2_times.argtypes = [vp, vp]
    L.rh_local_hp2_times.restype = ci
    L.rh_host_alloc.restype = vp
    L.rh_host_alloc.argtypes = [vp, ctypes.c_size_t]
    L.rh_host_free.restype = None
    L.rh_host_free.argtypes = [vp, vp]
    for f in ("rh_bpp", "rh_unpaired", "rh_fold", "rh_duplex", "rh_batch_upload", "rh_batch_compute", "rh_batch_results",
              "rh_batch_candidates", "rh_batch_timings", "rh_batch_device_views", "rh_batch_logz", "rh_batch_candidates_all",
              "rh_batch_layout", "rh_batch_results_all"):
        getattr(L, f).restype = ci
    _lib = L
    return L


def tri_size(n):
    return (n + 1) * (n + 2) // 2


def tri_offset(n, i):
    return i * (2 * (n + 1) - i - 1) // 2


def band_to_tri(bp_band):
    """The reference's triangular layout (tri_size(n) doubles, pair (i, j) 1-based at tri_offset(n, i) + j) of a band
    bp_band[i, d] = bp(i, i + d), 0-based i, as Context.local_fold returns it -- for n small enough to hold the triangle.  Pairs
    further apart than the band is wide are 0."""
    band = np.asarray(bp_band)
    n, ld = band.shape
    tri = np.zeros(tri_size(n), dtype=band.dtype)
    for i in range(n):
        m = min(ld - 1, n - 1 - i)
        at = tri_offset(n, i + 1) + i + 2
        tri[at:at + m] = band[i, 1:1 + m]
    return tri


def index_pairs(pairs):
    """(seqs, first, second) of a list of (s1, s2) pairs: identical strings once, in the order of their first appearance, and
    pair p = (seqs[first[p]], seqs[second[p]]) -- the arguments of Context.batch_upload_indexed."""
    slot, seqs, first, second = {}, [], [], []
    for a, b in pairs:
        for s, out in ((a, first), (b, second)):
            if s not in slot:
                slot[s] = len(seqs)
                seqs.append(s)
            out.append(slot[s])
    return seqs, first, second


def index_pairs_structured(pairs):
    """index_pairs for sequences that come with a structure line: pairs = [((s1, t1), (s2, t2)), ...], t = the line or "".
    Returns (seqs, structures, first, second); entries are distinct by (sequence, structure line), in the order of their first
    appearance -- one sequence under two lines is two entries, each folded under its own constraint."""
    slot, seqs, structures, first, second = {}, [], [], [], []
    for a, b in pairs:
        for (s, t), out in ((a, first), (b, second)):
            if (s, t) not in slot:
                slot[(s, t)] = len(seqs)
                seqs.append(s)
                structures.append(t)
            out.append(slot[(s, t)])
    return seqs, structures, first, second


class Context:
    """One rh_ctx: one GPU, one host thread."""

    def __init__(self, device=0, model=RH_MODEL_CONTRAFOLD, param_file=None, vienna=None):
        """vienna = dict(defaults_file=None, use_bl_param=True, semantics=0): rh_create_vienna (Vienna model only) -- the
        tables as RactIP::run installs them (library defaults -> BL* -> -P file) and the 1.8 / 2.x loop-energy semantics."""
        self.L = load_library()
        enc = lambda x: x.encode() if x else None
        if vienna is not None:
            if model != RH_MODEL_VIENNA_BL:
                raise RhError("vienna= applies to RH_MODEL_VIENNA_BL")
            self.h = self.L.rh_create_vienna(device, enc(vienna.get("defaults_file")), 1 if vienna.get("use_bl_param", True) else 0,
                                             enc(param_file), int(vienna.get("semantics", 0)))
        else:
            self.h = self.L.rh_create(device, model, enc(param_file))
        if not self.h:
            raise RhError("rh_create failed: %s" % self.L.rh_last_error(None).decode())
        self._pairs = []
        self._seq_lens = None   # lengths of the distinct sequences of an indexed upload (None: a plain one, 2 per pair)

    def vienna_semantics(self):
        """1 = ViennaRNA-1.8 loop energies, 2 = ViennaRNA-2.x (0: CONTRAfold model)."""
        return self.L.rh_vienna_semantics(self.h)

    def close(self):
        if getattr(self, "h", None):
            for ptr in getattr(self, "_pinned", []):
                self.L.rh_host_free(self.h, ptr)
            self._pinned = []
            self.L.rh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise RhError("ractip_hot error %d: %s" % (rc, self.L.rh_last_error(self.h).decode()))
        return rc

    def set_mode(self, mode):
        """0 = auto (linear, log-space fallback), 1 = log-space, 2 = linear only."""
        self._check(self.L.rh_set_mode(self.h, mode))

    def set_duplex_mode(self, mode):
        """Path of the pf_duplex sweeps alone: RH_MODE_INHERIT (-1, default: as set_mode says), 0 = auto, 1 = log-space, 2 = linear.
        Under the ViennaRNA-2.x semantics 0 / 2 run pf_duplex on the scaled linear kernels."""
        self._check(self.L.rh_set_duplex_mode(self.h, mode))

    def get_duplex_mode(self):
        return self.L.rh_get_duplex_mode(self.h)

    def last_path(self):
        return self.L.rh_last_path(self.h)

    def set_hybrid(self, cofold):
        """Vienna-BL model: hp from pf_duplex (False, default) or from the two-molecule ensemble of co_pf_fold (True)."""
        self._check(self.L.rh_set_hybrid(self.h, 1 if cofold else 0))

    def last_hybrid_path(self):
        return self.L.rh_last_hybrid_path(self.h)

    def set_max_w(self, max_w):
        self._check(self.L.rh_set_max_w(self.h, max_w))

    @property
    def max_w(self):
        return self.L.rh_get_max_w(self.h)

    def set_region_accessibility(self, on):
        """CONTRAfold model: accessibility of regions wider than one letter (off by default; see rh_set_region_accessibility)."""
        self._check(self.L.rh_set_region_accessibility(self.h, 1 if on else 0))

    @property
    def region_accessibility(self):
        return bool(self.L.rh_get_region_accessibility(self.h))

    def batch_acc_time(self):
        """Device time (ms) of the region-accessibility kernels of the last batch_compute (rh_batch_acc_time)."""
        ms = ctypes.c_double()
        self._check(self.L.rh_batch_acc_time(self.h, ctypes.byref(ms)))
        return ms.value

    # ---- single-problem calls
    def bpp(self, seq, constraint=None):
        n = len(seq)
        bp = np.zeros(tri_size(n))
        z = ctypes.c_double()
        self._check(self.L.rh_bpp(self.h, seq.encode(), n, constraint.encode() if constraint is not None else None,
                                  bp.ctypes.data, ctypes.addressof(z)))
        return bp, z.value

    def unpaired(self, seq, max_w=1):
        n = len(seq)
        up = np.zeros(n * max_w)
        self._check(self.L.rh_unpaired(self.h, seq.encode(), n, max_w, up.ctypes.data))
        return up.reshape(n, max_w)

    def fold(self, seq, constraint=None):
        n = len(seq)
        w = self.max_w
        bp, up, z = np.zeros(tri_size(n)), np.zeros(n * w), ctypes.c_double()
        if constraint is not None:
            self._check(self.L.rh_fold_constrained(self.h, seq.encode(), n, constraint.encode(), bp.ctypes.data, up.ctypes.data,
                                                   ctypes.addressof(z)))
        else:
            self._check(self.L.rh_fold(self.h, seq.encode(), n, bp.ctypes.data, up.ctypes.data, ctypes.addressof(z)))
        return bp, (up if w == 1 else up.reshape(n, w)), z.value

    def duplex(self, s1, s2):
        hp = np.zeros((len(s1) + 1, len(s2) + 1))
        z = ctypes.c_double()
        self._check(self.L.rh_duplex(self.h, s1.encode(), len(s1), s2.encode(), len(s2), hp.ctypes.data, ctypes.addressof(z)))
        return hp, z.value

    def cofold(self, s1, s2, constraint=None):
        """hp and log Z of the two-molecule ensemble, optionally under a constraint over s1+s2 (Vienna-BL model)."""
        hp = np.zeros((len(s1) + 1, len(s2) + 1))
        z = ctypes.c_double()
        self._check(self.L.rh_cofold_constrained(self.h, s1.encode(), len(s1), s2.encode(), len(s2),
                                                 constraint.encode() if constraint is not None else None, hp.ctypes.data, ctypes.addressof(z)))
        return hp, z.value

    # ---- local folding
    def local_fold(self, seq, window, step=1):
        """Window-averaged bp and accessibility of a long sequence (rh_local_fold): every window of `window` letters, one every
        `step` letters and a last one that ends at the last letter, is folded on its own, and each probability is the mean over the
        windows that contain it.  Returns (bp_band, up, logz, starts): bp_band (n, ld) with bp_band[i, d] = bp(i, i + d), 0-based,
        ld = min(window, n); up (n, max_w); log Z and start of every window.  band_to_tri gives the triangular layout."""
        self._check(self.L.rh_local_fold(self.h, seq.encode(), len(seq), window, step))
        return self.local_results()

    def local_results(self):
        """(bp_band, up, logz, starts) of the last local_fold, which stays fetchable until the next one (rh_local_results)."""
        n, ld, nw, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_local_layout(self.h, ctypes.byref(n), ctypes.byref(ld), ctypes.byref(nw), ctypes.byref(w), None))
        band, up = np.empty((n.value, ld.value)), np.empty((n.value, w.value))
        logz, starts = np.empty(nw.value), np.empty(nw.value, dtype=np.int32)
        self._check(self.L.rh_local_layout(self.h, None, None, None, None, starts.ctypes.data))
        self._check(self.L.rh_local_results(self.h, band.ctypes.data, up.ctypes.data, logz.ctypes.data))
        return band, up, logz, starts

    def local_duplex(self, s1, s2, window, step=1, windowed=2):
        """Window-averaged hybridization matrix of a query on a long target (rh_local_duplex): molecule `windowed` (1 or 2) is cut into
        the windows of local_fold, the other one is whole, and every window is hybridized with it under the context's settings.
        Returns (hp, logz_pair, starts): hp (n1+1, n2+1), 1-based, the mean over the windows that contain the windowed molecule's
        letter; log Z of every window pair; the window starts.  The call is also local_fold of the windowed molecule
        (local_results), and it leaves the last chunk as the context's batch: query + windows, indexed."""
        self._check(self.L.rh_local_duplex(self.h, s1.encode(), len(s1), s2.encode(), len(s2), windowed, window, step))
        ns, index = self.batch_index()
        nq, we = (len(s1), min(window, len(s2))) if windowed == 2 else (len(s2), min(window, len(s1)))
        self._seq_lens = [nq] + [we] * (ns - 1)
        self._pairs = [(self._seq_lens[a], self._seq_lens[b]) for a, b in index]
        hp, logz = self.local_hp_results()
        starts = np.empty(logz.shape[0], dtype=np.int32)
        self._check(self.L.rh_local_layout(self.h, None, None, None, None, starts.ctypes.data))
        return hp, logz, starts

    def local_hp_results(self):
        """(hp, logz_pair) of the last local_duplex (rh_local_hp_results); a later local_fold drops them."""
        n1, n2, nw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_local_hp_layout(self.h, ctypes.byref(n1), ctypes.byref(n2), None, ctypes.byref(nw)))
        hp, logz = np.empty((n1.value + 1, n2.value + 1)), np.empty(nw.value)
        self._check(self.L.rh_local_hp_results(self.h, hp.ctypes.data, logz.ctypes.data))
        return hp, logz

    def local_candidates(self, what, threshold, cap=1 << 22):
        """Thresholded list of the last local_fold, scanned on the device (rh_local_candidates): what = 0 the pairs (1-based i < j),
        1 the accessibilities (0-based position, width index), 2 the hybridization matrix of the last local_duplex (1-based letters
        of s1 and s2).  Returns (records, total): a structured array (i, j, p) of
        min(total, cap) records in row-major order, and the number found."""
        buf = np.empty(max(cap, 1), dtype=self.CAND_DTYPE)
        k = self._check(self.L.rh_local_candidates(self.h, what, ctypes.c_float(threshold), buf.ctypes.data, cap))
        return buf[:min(k, cap)], k

    def set_local_chunk(self, windows):
        """Windows per chunk of local_fold (0: automatic, by the byte budget of the McCaskill tables); results are unchanged."""
        self._check(self.L.rh_set_local_chunk(self.h, windows))

    def local_times(self):
        """Device time (ms) of the last local_fold: (folds, accumulate + finish + the scans since)."""
        ms = (ctypes.c_double * 2)()
        self._check(self.L.rh_local_times(self.h, ms))
        return ms[0], ms[1]

    # ---- span-limited folding
    def set_span_contrafold(self, on):
        """CONTRAfold model: span_fold and span_fold_batch on this context (off by default, when a CONTRAfold context refuses them;
        see rh_set_span_contrafold).  Accepted on a Vienna-BL context, where it changes nothing."""
        self._check(self.L.rh_set_span_contrafold(self.h, 1 if on else 0))

    def get_span_contrafold(self):
        return bool(self.L.rh_get_span_contrafold(self.h))

    def span_fold(self, seq, max_span, max_w=1, constraint=None):
        """The McCaskill ensemble of the whole sequence restricted to pairs (a, b) with b - a < max_span (rh_span_fold_acc; Vienna-BL
        contexts, 1.8 semantics, and CONTRAfold contexts after set_span_contrafold(True), there without a constraint, pairs of
        complementary letters, and max_w > 1 only after set_region_accessibility(True)): one partition function, O(n L) memory.  Returns (bp_band, up, logz): bp_band (n, ld) with
        bp_band[i, d] = P(i, i + d), 0-based, ld = min(max_span, n); up (n, max_w) with up[i, w] = P(letters i .. i + w unpaired),
        0-based, 0 where the run passes the end (max_w in 1..64; the context's own max_w is not used); log Z of the whole sequence.
        The result is the context's local result (local_results, local_candidates); band_to_tri gives the triangular layout.
        constraint: a string in the fold_constrained alphabet of bpp, which restricts the pairs further (rh_span_fold_constrained);
        a matched bracket pair must lie within max_span."""
        if constraint is not None:
            self._check(self.L.rh_span_fold_constrained(self.h, seq.encode(), len(seq), constraint.encode(), max_span, max_w))
        else:
            self._check(self.L.rh_span_fold_acc(self.h, seq.encode(), len(seq), max_span, max_w))
        band, up, logz, _ = self.local_results()
        return band, up, float(logz[0])

    def span_times(self):
        """Device time (ms) of the last span_fold: (inside + outside sweeps, exterior passes + finish)."""
        ms = (ctypes.c_double * 2)()
        self._check(self.L.rh_span_times(self.h, ms))
        return ms[0], ms[1]

    def span_acc_times(self):
        """Device time (ms) of the accessibility stage of the last span_fold at max_w > 1: (hairpin part, gap sums, final kernel);
        on a CONTRAfold context (everything but the multiloop chain, the chain's S build, its links and closes)."""
        ms = (ctypes.c_double * 3)()
        self._check(self.L.rh_span_acc_times(self.h, ms))
        return ms[0], ms[1], ms[2]

    def span_fold_batch(self, seqs, max_span, max_w=1, constraints=None):
        """span_fold of every sequence of `seqs` (ragged lengths) through one set of launches (rh_span_fold_batch): a list of
        (bp_band, up, logz), item k with the bits of span_fold(seqs[k], max_span, max_w) on this context.  The result lives beside the
        local result until the next span_fold_batch (span_batch_results, span_batch_candidates).  Raises for an item for which no
        scale exponent of the ladder holds, and names it.  Contexts as for span_fold: a CONTRAfold context needs
        set_span_contrafold(True), no constraints and, for max_w > 1, set_region_accessibility(True).
        constraints: one string or None per sequence (rh_span_fold_batch_constrained); item k then has the bits of
        span_fold(seqs[k], max_span, max_w, constraints[k])."""
        enc = [s.encode() for s in seqs]
        arr = (ctypes.c_char_p * max(len(enc), 1))(*enc)
        lens = (ctypes.c_int * max(len(enc), 1))(*[len(s) for s in seqs])
        if constraints is not None:
            if len(constraints) != len(enc):
                raise RhError("%d constraints for %d sequences" % (len(constraints), len(enc)))
            cons = (ctypes.c_char_p * max(len(enc), 1))(*[None if x is None else x.encode() for x in constraints])
            self._check(self.L.rh_span_fold_batch_constrained(self.h, arr, lens, len(enc), cons, max_span, max_w))
        else:
            self._check(self.L.rh_span_fold_batch(self.h, arr, lens, len(enc), max_span, max_w))
        return [self.span_batch_results(k) for k in range(len(enc))]

    def span_batch_results(self, item):
        """(bp_band, up, logz) of one item of the last span_fold_batch (rh_span_batch_item, rh_span_batch_results)."""
        n, ld, status, w = (ctypes.c_int() for _ in range(4))
        self._check(self.L.rh_span_batch_layout(self.h, None, None, ctypes.byref(w)))
        self._check(self.L.rh_span_batch_item(self.h, item, ctypes.byref(n), ctypes.byref(ld), ctypes.byref(status)))
        band, up, logz = np.empty((n.value, ld.value)), np.empty((n.value, w.value)), np.empty(1)
        self._check(self.L.rh_span_batch_results(self.h, item, band.ctypes.data, up.ctypes.data, logz.ctypes.data))
        return band, up, float(logz[0])

    def span_batch_candidates(self, item, what, threshold, cap=1 << 22):
        """Thresholded list of one item of the last span_fold_batch (rh_span_batch_candidates): what = 0 the pairs, 1 the
        accessibilities; (records, total) as local_candidates returns them after the item's single span_fold."""
        buf = np.empty(max(cap, 1), dtype=self.CAND_DTYPE)
        k = self._check(self.L.rh_span_batch_candidates(self.h, item, what, ctypes.c_float(threshold), buf.ctypes.data, cap))
        return buf[:min(k, cap)], k

    def set_span_batch_bytes(self, b):
        """Table memory (bytes) one chunk of a span_fold_batch may take (0: the default, 16 GiB); results are unchanged."""
        self._check(self.L.rh_set_span_batch_bytes(self.h, b))

    def span_batch_times(self):
        """Device time (ms) of the last span_fold_batch, summed over chunks and ladder attempts: (sweeps, exterior passes + finish,
        accessibility stage)."""
        ms = (ctypes.c_double * 3)()
        self._check(self.L.rh_span_batch_times(self.h, ms))
        return ms[0], ms[1], ms[2]

    # ---- local hybridization of two windowed molecules
    def local_duplex2(self, s1, s2, window1, step1=1, window2=None, step2=None):
        """Window-averaged hybridization matrix of two long molecules (rh_local_duplex2): s1 is cut into windows (window1, step1), s2
        into (window2, step2) -- by default the same pair -- and every window of s1 is hybridized with every window of s2 under the
        context's settings.  Returns (hp, logz_pair, starts1, starts2): hp (n1+1, n2+1), 1-based, per entry the sum over the windows
        of s1 that contain the row's letter, in increasing order, of the sums over the windows of s2 that contain the column's letter,
        divided once by the product of the two counts; log Z of every window pair, (nw1, nw2); the window starts.  The result stays
        fetchable until the next local_duplex2, whatever local_fold and local_duplex do meanwhile.  The call leaves its last tile as the
        context's batch: the tile's windows of s1, then those of s2, indexed."""
        window2 = window1 if window2 is None else window2
        step2 = step1 if step2 is None else step2
        self._check(self.L.rh_local_duplex2(self.h, s1.encode(), len(s1), s2.encode(), len(s2), window1, step1, window2, step2))
        ns, index = self.batch_index()
        rows = index[0][1] if index else 0                      # pair 0 = (0, rows)
        self._seq_lens = [min(window1, len(s1))] * rows + [min(window2, len(s2))] * (ns - rows)
        self._pairs = [(self._seq_lens[a], self._seq_lens[b]) for a, b in index]
        return self.local_hp2_results()

    def local_hp2_results(self):
        """(hp, logz_pair (nw1, nw2), starts1, starts2) of the last local_duplex2 (rh_local_hp2_results)."""
        n1, n2, nw1, nw2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_local_hp2_layout(self.h, ctypes.byref(n1), ctypes.byref(n2), ctypes.byref(nw1), ctypes.byref(nw2), None, None))
        hp, logz = np.empty((n1.value + 1, n2.value + 1)), np.empty((nw1.value, nw2.value))
        starts1, starts2 = np.empty(nw1.value, dtype=np.int32), np.empty(nw2.value, dtype=np.int32)
        self._check(self.L.rh_local_hp2_layout(self.h, None, None, None, None, starts1.ctypes.data, starts2.ctypes.data))
        self._check(self.L.rh_local_hp2_results(self.h, hp.ctypes.data, logz.ctypes.data))
        return hp, logz, starts1, starts2

    def local_hp2_candidates(self, threshold, cap=1 << 22):
        """Thresholded list of the last local_duplex2's hp, scanned on the device (rh_local_hp2_candidates): (records, total) as
        local_candidates(2, ...) returns them, 1-based letters of s1 and s2 in row-major order."""
        buf = np.empty(max(cap, 1), dtype=self.CAND_DTYPE)
        k = self._check(self.L.rh_local_hp2_candidates(self.h, ctypes.c_float(threshold), buf.ctypes.data, cap))
        return buf[:min(k, cap)], k

    def set_local_tile(self, rows, cols):
        """Windows of s1 x windows of s2 per tile of local_duplex2 ((0, 0): automatic, by the byte budget); results are unchanged."""
        self._check(self.L.rh_set_local_tile(self.h, rows, cols))

    def local_hp2_tile(self):
        """(rows, cols) of the tile the last local_duplex2 ran."""
        rows, cols = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_local_hp2_tile(self.h, ctypes.byref(rows), ctypes.byref(cols)))
        return rows.value, cols.value

    def local_hp2_times(self):
        """Device time (ms) of the last local_duplex2: (the tiles' computes, row + add + finish kernels and the scans since)."""
        ms = (ctypes.c_double * 2)()
        self._check(self.L.rh_local_hp2_times(self.h, ms))
        return ms[0], ms[1]

    # ---- batched calls
    def batch_upload(self, pairs, constraints=None, co_constraints=None):
        """constraints: per pair (c1, c2), the fold_constrained strings of the two single-molecule folds (either may be None);
        co_constraints: per pair a string over s1+s2 for the two-molecule ensemble, or None (rh_batch_upload_constrained)."""
        np_ = len(pairs)
        a = (ctypes.c_char_p * np_)(*[p[0].encode() for p in pairs])
        b = (ctypes.c_char_p * np_)(*[p[1].encode() for p in pairs])
        na = (ctypes.c_int * np_)(*[len(p[0]) for p in pairs])
        nb = (ctypes.c_int * np_)(*[len(p[1]) for p in pairs])
        if constraints is None and co_constraints is None:
            self._check(self.L.rh_batch_upload(self.h, np_, a, na, b, nb))
        else:
            def column(strings):
                if strings is None:
                    return None
                if len(strings) != np_:
                    raise RhError("%d constraints for %d pairs" % (len(strings), np_))
                return (ctypes.c_char_p * np_)(*[None if x is None else x.encode() for x in strings])
            pairs_c = None if constraints is None else [c if c is not None else (None, None) for c in constraints]
            c1 = column(None if pairs_c is None else [c[0] for c in pairs_c])
            c2 = column(None if pairs_c is None else [c[1] for c in pairs_c])
            self._check(self.L.rh_batch_upload_constrained(self.h, np_, a, na, b, nb, c1, c2, column(co_constraints)))
        self._pairs = [(len(p[0]), len(p[1])) for p in pairs]
        self._seq_lens = None

    def batch_upload_indexed(self, seqs, index_pairs, constraints=None, co_first=None, co_second=None):
        """Every string of `seqs` is folded once; pair p = (seqs[i], seqs[j]) for (i, j) = index_pairs[p] (rh_batch_upload_indexed).
        The per-pair calls (batch_results, batch_candidates, batch_candidates_all, batch_logz) work as on the expanded batch.
        constraints / co_first / co_second (rh_batch_upload_indexed_constrained, Vienna-BL model): one string or None per entry
        of `seqs` -- the constraint of its fold, and its share of a pair's joint constraint when it is s1 / s2 of the pair."""
        ns, np_ = len(seqs), len(index_pairs)
        a = (ctypes.c_char_p * ns)(*[s.encode() for s in seqs])
        na = (ctypes.c_int * ns)(*[len(s) for s in seqs])
        first = (ctypes.c_int * max(np_, 1))(*[int(p[0]) for p in index_pairs])
        second = (ctypes.c_int * max(np_, 1))(*[int(p[1]) for p in index_pairs])
        if constraints is None and co_first is None and co_second is None:
            self._check(self.L.rh_batch_upload_indexed(self.h, ns, a, na, np_, first, second))
        else:
            def column(strings):
                if strings is None:
                    return None
                if len(strings) != ns:
                    raise RhError("%d constraints for %d sequences" % (len(strings), ns))
                return (ctypes.c_char_p * ns)(*[None if x is None else x.encode() for x in strings])
            self._check(self.L.rh_batch_upload_indexed_constrained(self.h, ns, a, na, np_, first, second, column(constraints),
                                                                   column(co_first), column(co_second)))
        self._pairs = [(len(seqs[p[0]]), len(seqs[p[1]])) for p in index_pairs]
        self._seq_lens = [len(s) for s in seqs]

    def batch_index(self):
        """(nseq, [(first, second)] per pair) of the last upload; for batch_upload: nseq = 2 npairs and the pairs (2p, 2p+1)."""
        ns, np_ = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_batch_index(self.h, ctypes.byref(ns), ctypes.byref(np_), None, None))
        first, second = (ctypes.c_int * max(np_.value, 1))(), (ctypes.c_int * max(np_.value, 1))()
        self._check(self.L.rh_batch_index(self.h, None, None, first, second))
        return ns.value, [(first[p], second[p]) for p in range(np_.value)]

    def batch_candidates_seq_all(self, what, threshold, cap=1 << 22):
        """Candidates per DISTINCT sequence: what = 0 the bp lists, 1 the up lists (records, first) with nseq+1 offsets -- the form of
        batch_candidates_all that does not repeat a sequence's list for every pair that uses it."""
        if getattr(self, "_cand_buf", None) is None or self._cand_buf.size < cap:
            self._cand_buf = np.empty(cap, dtype=self.CAND_DTYPE)
        ns = len(self._seq_lens) if self._seq_lens is not None else 2 * len(self._pairs)
        first = np.empty(ns + 1, dtype=np.int32)
        k = self._check(self.L.rh_batch_candidates_seq_all(self.h, what, ctypes.c_float(threshold), self._cand_buf.ctypes.data,
                                                           cap, first.ctypes.data))
        if k > cap:
            raise RhError("candidate buffer too small: %d > %d" % (k, cap))
        return self._cand_buf[:k], first

    def debug_allow_mask(self, which, k):
        """The allowed-pair mask of the last upload as the kernels read it (rh_debug_batch_allow_mask): which = 0, sequence k
        (2p = s1 of pair p; indexed upload: distinct sequence k), which = 1 the concatenation of pair k.  An (ld, ld) uint8 array, or None if that batch has no mask."""
        ld = ctypes.c_int()
        if self._check(self.L.rh_debug_batch_allow_mask(self.h, which, k, None, ctypes.byref(ld))) == 1:
            return None
        out = np.empty((ld.value, ld.value), dtype=np.uint8)
        self._check(self.L.rh_debug_batch_allow_mask(self.h, which, k, out.ctypes.data, ctypes.byref(ld)))
        return out

    def batch_compute(self):
        self._check(self.L.rh_batch_compute(self.h))

    def batch_results(self, p):
        n1, n2 = self._pairs[p]
        bp1, bp2 = np.zeros(tri_size(n1)), np.zeros(tri_size(n2))
        w = self.max_w
        up1, up2 = np.zeros(n1 * w), np.zeros(n2 * w)
        hp = np.zeros((n1 + 1, n2 + 1))
        z3 = np.zeros(3)
        self._check(self.L.rh_batch_results(self.h, p, bp1.ctypes.data, bp2.ctypes.data, up1.ctypes.data,
                                            up2.ctypes.data, hp.ctypes.data, z3.ctypes.data))
        if w > 1:
            up1, up2 = up1.reshape(n1, w), up2.reshape(n2, w)
        return dict(bp1=bp1, bp2=bp2, up1=up1, up2=up2, hp=hp, logZ=z3)

    def batch_logz(self):
        out = np.zeros((len(self._pairs), 3))
        self._check(self.L.rh_batch_logz(self.h, out.ctypes.data))
        return out

    def batch_candidates(self, p, which, threshold, cap=1 << 20):
        buf = (Cand * cap)()
        k = self._check(self.L.rh_batch_candidates(self.h, p, which, ctypes.c_float(threshold), buf, cap))
        self.last_candidate_count = k
        return [(buf[t].i, buf[t].j, buf[t].p) for t in range(min(k, cap))]

    CAND_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("p", np.float32)])

    def batch_candidates_all(self, which, threshold, cap=1 << 22):
        """Candidates of every pair: (records, first) -- a structured array (i, j, p) and the np+1 offsets
        such that pair k owns records[first[k]:first[k+1]].  No per-entry Python work."""
        if getattr(self, "_cand_buf", None) is None or self._cand_buf.size < cap:
            self._cand_buf = np.empty(cap, dtype=self.CAND_DTYPE)
        first = np.empty(len(self._pairs) + 1, dtype=np.int32)
        k = self._check(self.L.rh_batch_candidates_all(self.h, which, ctypes.c_float(threshold), self._cand_buf.ctypes.data,
                                                       cap, first.ctypes.data))
        if k > cap:
            raise RhError("candidate buffer too small: %d > %d" % (k, cap))
        return self._cand_buf[:k], first

    def batch_results_all(self):
        """Dense results of all pairs (three device-to-host copies), unpacked into per-pair dicts.  After batch_upload_indexed the
        folds are per distinct sequence: one dict(bp=[nseq tables], up=[nseq], hp=[npairs matrices], logZ=(npairs, 3))."""
        ts, hs = ctypes.c_size_t(), ctypes.c_size_t()
        uld, hld = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_batch_layout(self.h, ctypes.byref(ts), ctypes.byref(uld), ctypes.byref(hs), ctypes.byref(hld)))
        np_ = len(self._pairs)
        if getattr(self, "_seq_lens", None) is not None:
            lens, w = self._seq_lens, self.max_w
            bp = np.empty((len(lens), ts.value)); up = np.empty((len(lens), uld.value)); hp = np.empty((np_, hs.value)); z = np.empty((np_, 3))
            self._check(self.L.rh_batch_results_all(self.h, bp.ctypes.data, up.ctypes.data, hp.ctypes.data, z.ctypes.data))
            return dict(bp=[bp[k][:tri_size(n)] for k, n in enumerate(lens)],
                        up=[up[k][:n * w] if w == 1 else up[k][:n * w].reshape(n, w) for k, n in enumerate(lens)],
                        hp=[hp[p][:(n1 + 1) * hld.value].reshape(n1 + 1, hld.value)[:, :n2 + 1] for p, (n1, n2) in enumerate(self._pairs)],
                        logZ=z)
        bp = np.empty((2 * np_, ts.value)); up = np.empty((2 * np_, uld.value)); hp = np.empty((np_, hs.value)); z = np.empty((np_, 3))
        self._check(self.L.rh_batch_results_all(self.h, bp.ctypes.data, up.ctypes.data, hp.ctypes.data, z.ctypes.data))
        out = []
        w = self.max_w
        for p, (n1, n2) in enumerate(self._pairs):
            h = hp[p][:(n1 + 1) * hld.value].reshape(n1 + 1, hld.value)[:, :n2 + 1]
            u1, u2 = up[2 * p][:n1 * w], up[2 * p + 1][:n2 * w]
            if w > 1:
                u1, u2 = u1.reshape(n1, w), u2.reshape(n2, w)
            out.append(dict(bp1=bp[2 * p][:tri_size(n1)], bp2=bp[2 * p + 1][:tri_size(n2)], up1=u1, up2=u2, hp=h, logZ=z[p]))
        return out

    def pinned_empty(self, shape, dtype=np.float64):
        """numpy array over page-locked host memory (rh_host_alloc).  The memory belongs to the context: it is released by
        pinned_free(array) or close(), and the array must not be touched afterwards."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.L.rh_host_alloc(self.h, max(nbytes, 8))
        if not ptr:
            raise RhError("rh_host_alloc failed: %s" % self.L.rh_last_error(self.h).decode())
        self._pinned = getattr(self, "_pinned", []) + [ptr]
        buf = (ctypes.c_char * max(nbytes, 8)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def pinned_free(self, arr):
        """Release one pinned_empty array now (rh_host_free) instead of with the context."""
        ptr = arr.ctypes.data
        pinned = getattr(self, "_pinned", [])
        if ptr in pinned:
            pinned.remove(ptr)
            self.L.rh_host_free(self.h, ptr)

    def batch_results_all_into(self, bufs=None):
        """Dense results of all pairs in the padded device layout (rh_batch_layout), three copies, no unpacking.  `bufs` =
        (bp, up, hp, logz) arrays from a previous call are reused when the layout is unchanged; they are page-locked."""
        ts, hs = ctypes.c_size_t(), ctypes.c_size_t()
        uld, hld = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.rh_batch_layout(self.h, ctypes.byref(ts), ctypes.byref(uld), ctypes.byref(hs), ctypes.byref(hld)))
        np_ = len(self._pairs)
        ns = len(self._seq_lens) if getattr(self, "_seq_lens", None) is not None else 2 * np_
        shapes = ((ns, ts.value), (ns, uld.value), (np_, hs.value), (np_, 3))
        if bufs is None or tuple(b.shape for b in bufs) != shapes:
            for b in bufs or ():          # the layout changed: the buffers this call replaces are released, not kept until close()
                self.pinned_free(b)
            bufs = tuple(self.pinned_empty(sh) for sh in shapes)
        self._check(self.L.rh_batch_results_all(self.h, *[b.ctypes.data for b in bufs]))
        return bufs

    def batch_packed_layout(self):
        """(bp_off, up_off, hp_off, totals) of the packed float image of the last upload (rh_batch_packed_layout): element offsets as
        uint64 arrays of nseq+1, nseq+1 and npairs+1 entries, and the three totals.  Valid after the upload, before the compute."""
        np_ = len(self._pairs)
        ns = len(self._seq_lens) if getattr(self, "_seq_lens", None) is not None else 2 * np_
        bo, uo, ho = np.zeros(ns + 1, dtype=np.uint64), np.zeros(ns + 1, dtype=np.uint64), np.zeros(np_ + 1, dtype=np.uint64)
        tot = np.zeros(3, dtype=np.uint64)
        self._check(self.L.rh_batch_packed_layout(self.h, bo.ctypes.data, uo.ctypes.data, ho.ctypes.data, tot.ctypes.data))
        return bo, uo, ho, tot

    def batch_results_packed_f32(self, bufs=None, want=("bp", "up", "hp", "logz")):
        """Dense results of the whole batch as float32, narrowed and packed on the device (rh_batch_results_packed_f32): half the bytes
        of batch_results_all_into, no host conversion.  Returns dict(bp=[per sequence], up=[per sequence], hp=[per pair], logZ=(npairs, 3),
        bufs=(bp, up, hp, logz)): the lists hold views -- slices, not copies -- of the page-locked float32 buffers `bufs`, which a
        later call reuses when handed back with unchanged totals.  Sequences are 2p = s1, 2p+1 = s2 of pair p, or the distinct ones of an
        indexed upload; hp[p] is (n1+1, n2+1), up[k] is (n, max_w) when max_w > 1.  A kind not named in `want` is not fetched (NULL
        to the C call) and its buffer keeps what it held."""
        bo, uo, ho, tot = self.batch_packed_layout()
        np_, w = len(self._pairs), self.max_w
        lens = self._seq_lens if getattr(self, "_seq_lens", None) is not None else [n for pr in self._pairs for n in pr]
        shapes = ((int(tot[0]),), (int(tot[1]),), (int(tot[2]),), (np_, 3))
        if bufs is None or tuple(b.shape for b in bufs) != shapes:
            for b in bufs or ():          # the totals changed: the buffers this call replaces are released, not kept until close()
                self.pinned_free(b)
            bufs = tuple(self.pinned_empty(sh, np.float32 if k < 3 else np.float64) for k, sh in enumerate(shapes))
        ptr = [b.ctypes.data if name in want else None for b, name in zip(bufs, ("bp", "up", "hp", "logz"))]
        self._check(self.L.rh_batch_results_packed_f32(self.h, *ptr))
        bp, up, hp, z = bufs
        ups = [up[int(uo[k]):int(uo[k]) + n * w] for k, n in enumerate(lens)]
        return dict(bp=[bp[int(bo[k]):int(bo[k]) + tri_size(n)] for k, n in enumerate(lens)],
                    up=ups if w == 1 else [u.reshape(n, w) for u, n in zip(ups, lens)],
                    hp=[hp[int(ho[p]):int(ho[p]) + (n1 + 1) * (n2 + 1)].reshape(n1 + 1, n2 + 1) for p, (n1, n2) in enumerate(self._pairs)],
                    logZ=z, bufs=bufs)

    def batch_pack_time(self):
        """Device time (ms) of the pack kernel of the last batch_results_packed_f32 (rh_batch_pack_time)."""
        ms = ctypes.c_double()
        self._check(self.L.rh_batch_pack_time(self.h, ctypes.byref(ms)))
        return ms.value

    def batch_fallbacks(self, which=0):
        """Indices of the sequences (which=0) / pairs (which=1) the last compute recomputed in log space; which=2: the sequences it
        recomputed on the linear kernels with another scale exponent; which=3: the pairs whose duplex sweeps it recomputed that way."""
        buf = (ctypes.c_int * max(1, 2 * len(self._pairs)))()
        k = self._check(self.L.rh_batch_fallbacks(self.h, which, buf, len(buf)))
        return [buf[t] for t in range(min(k, len(buf)))]

    def set_scale_memory(self, on):
        """True: the next batch starts on the scale exponent most of the last one needed (faster on streams of one kind of input;
        a sequence's bits then depend on the context's history).  Default off."""
        self._check(self.L.rh_set_scale_memory(self.h, 1 if on else 0))

    def kernel_class_times(self, cls, computes=1):
        """Average duration (us) and launches per compute of ONE class of sweep kernels (rh_set_kernel_timing: 0 inside sweep kernel,
        1 its block products + packing, 2 outside sweep kernel, 3 its block products, 4 duplex sweep kernel), measured live with HIP
        event pairs around every launch of that class over `computes` passes of the current batch, phases not overlapping."""
        self._check(self.L.rh_set_kernel_timing(self.h, cls))
        self._check(self.L.rh_set_overlap(self.h, 0))
        n_tot, ms_tot = 0, 0.0
        try:
            for _ in range(computes):
                self.batch_compute()
                n, ms = ctypes.c_int(), ctypes.c_double()
                self._check(self.L.rh_kernel_times(self.h, ctypes.byref(n), ctypes.byref(ms)))
                n_tot += n.value
                ms_tot += ms.value
        finally:
            self.L.rh_set_kernel_timing(self.h, -1)
            self.L.rh_set_overlap(self.h, 1)
        return (ms_tot * 1e3 / n_tot if n_tot else 0.0), n_tot / float(computes)

    def set_overlap(self, on):
        """False: phases run one after the other (isolated per-phase device times in batch_timings)."""
        self._check(self.L.rh_set_overlap(self.h, 1 if on else 0))

    def batch_kernels(self):
        """[(per-diagonal kernel, block-product kernel or '', block-product launches)] for inside, outside, duplex."""
        fine, far, nf = (ctypes.c_char_p * 3)(), (ctypes.c_char_p * 3)(), (ctypes.c_int * 3)()
        self._check(self.L.rh_batch_kernels(self.h, fine, far, nf))
        return [((fine[k] or b"").decode(), (far[k] or b"").decode(), nf[k]) for k in range(3)]

    def batch_timings(self):
        ms = (ctypes.c_double * 4)()
        nl = (ctypes.c_int * 3)()
        self._check(self.L.rh_batch_timings(self.h, ms, nl))
        return list(ms), list(nl)
