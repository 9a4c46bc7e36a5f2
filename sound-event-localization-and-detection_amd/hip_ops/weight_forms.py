"""Packed weight forms of the 8-multiplication Hamilton product kernels (csrc/hcq_conv.hip): the packing entry points and
the cache that rebuilds the forms when the weights change instead of per call."""
import ctypes
import weakref

import numpy as np
import torch

from .. import _lib as L
from ._core import _req, memo


def hcq_pack_floats(desc, mode, nsets=1):
    """Floats of the packed weight-form buffer, 0 if the fast-product kernel does not take this shape."""
    return int(L.lib().seld_hcq_pack_floats(ctypes.byref(desc), int(mode), int(nsets)))


@memo
def _hcq_ok(desc, mode, npair=1):
    """Does the fast-product kernel take this (shape, direction)?  (cached; no weights needed)"""
    return desc.algebra > 1 and hcq_pack_floats(desc, mode, npair) > 0


def hcq_pack(desc, mode, wsA, wsB=None, out=None):
    """Weight forms F_m(W) in MFMA fragment order (seld_hcq_pack): mode 0 forward, 1 data gradient."""
    nsets = 2 if wsB is not None else 1
    n = hcq_pack_floats(desc, mode, nsets)
    if n == 0:
        return None
    if out is None:
        out = torch.empty(n, device=wsA[0].device, dtype=torch.float32)
    L.check(L.lib().seld_hcq_pack(ctypes.byref(desc), int(mode), nsets, L.ptr_array8([_req(w, "w") for w in wsA]),
                                  L.ptr_array8([_req(w, "w") for w in wsB]) if wsB is not None else None, L.ptr(out),
                                  L.current_stream()), "seld_hcq_pack")
    return out


class _HcqWeights:
    """Packed weight forms of every (layer, direction) that runs on the fast-product kernels.

    The forms depend on the weights only, so they are rebuilt when the weights change, not per call:
      * `weights_changed()` (FlatAdam.step, anything that rewrites parameters behind torch's back) starts a new epoch;
        the first request of an epoch re-packs EVERY registered entry in one launch (seld_hcq_pack_flat);
      * an in-place edit torch knows about (load_state_dict, an eager optimiser) shows in the tensors' version counters
        and re-packs just the entry that is asked for;
      * parameters that moved (Module.to, FlatAdam re-homing them into its flat buffer) are noticed by their pointers.
    Entries hold weak references: a deleted model drops out at the next full re-pack."""

    def __init__(self):
        self.entries = {}
        self.epoch = 0
        self._esize = None
        self.reset()

    def weights_changed(self):
        self.epoch += 1

    def reset(self):
        self.entries.clear()
        self.table, self.table_dirty, self.packed_epoch = None, True, -1
        self.starts, self.total_blocks = None, 0

    def repack_pending(self):
        """Will the next request re-pack every registered entry (the weights changed since the last full re-pack)?"""
        return self.packed_epoch != self.epoch

    def ensure_packed(self):
        """Do that re-pack now, on the current stream, if it is pending."""
        if self.repack_pending():
            self._pack_all()

    class _Entry:
        __slots__ = ("desc", "mode", "refs", "npair", "nA", "buf", "ptrs", "vers", "epoch", "host")

    @staticmethod
    def _alive(e):
        ws = [r() for r in e.refs]
        return None if any(w is None for w in ws) else ws

    def _fill(self, e, ws):
        """(Re)build the table entry of `e` from the weights' current addresses."""
        lib = L.lib()
        if self._esize is None:
            self._esize = int(lib.seld_hcq_pack_entry_bytes())
        host = ctypes.create_string_buffer(self._esize)
        wsA, wsB = ws[:e.nA], (ws[e.nA:] if e.npair == 2 else None)
        L.check(lib.seld_hcq_pack_entry(ctypes.byref(e.desc), e.mode, e.npair, L.ptr_array8(wsA),
                                        L.ptr_array8(wsB) if wsB is not None else None, L.ptr(e.buf), host),
                "seld_hcq_pack_entry")
        e.host = host.raw
        e.ptrs = tuple(w.data_ptr() for w in ws)
        e.vers = None
        e.epoch = -1
        self.table_dirty = True

    def refresh_table(self):
        """Bring the device-side table up to date with the registered entries WITHOUT packing (host work + two small
        host-to-device copies).  step.GraphedTrainStep calls it right before recording: entries registered during the
        warm-up step left the table dirty, and the copies are not allowed inside a stream capture."""
        return self._collect()[0]

    def _collect(self):
        dead = []
        versions = {}
        for key, e in self.entries.items():
            if e is None:
                continue
            ws = self._alive(e)
            if ws is None or any(not w.is_cuda for w in ws):
                dead.append(key)
                continue
            if tuple(w.data_ptr() for w in ws) != e.ptrs:
                self._fill(e, ws)
            versions[id(e)] = tuple(w._version for w in ws)
        for key in dead:
            del self.entries[key]
            self.table_dirty = True
        live = [e for e in self.entries.values() if e is not None]
        if live and self.table_dirty:
            raw = b"".join(e.host for e in live)
            self.table = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(live[0].buf.device)
            starts = np.zeros(len(live) + 1, dtype=np.int32)
            starts[1:] = np.cumsum([(e.buf.numel() + 255) // 256 for e in live])
            self.starts = torch.from_numpy(starts).to(live[0].buf.device)
            self.total_blocks = int(starts[-1])
            self.table_dirty = False
        return live, versions

    def _pack_all(self):
        live, versions = self._collect()
        if not live:
            self.packed_epoch = self.epoch
            return
        L.check(L.lib().seld_hcq_pack_flat(L.ptr(self.table), L.ptr(self.starts), len(live), self.total_blocks,
                                           L.current_stream()), "seld_hcq_pack_flat")
        # the version counters the forms were built from: an in-place edit torch knows about (load_state_dict) between now
        # and the entry's next request shows as a mismatch there and re-packs that entry (with None recorded
        # here, an entry that was bulk-packed and then edited was served stale)
        for e in live:
            e.epoch, e.vers = self.epoch, versions[id(e)]
        self.packed_epoch = self.epoch

    def pin_for_graph(self):
        """Everything a RECORDED seld_hcq_pack_flat launch points at: the table, the block starts and the entries' form
        buffers as they are now.  `_pack_all` never edits a table in place -- it builds new tensors when an entry is added
        -- so a recorded step that holds these references keeps replaying against valid memory whatever shapes are
        registered later (validation at another batch size, an eval-only pooling entry)."""
        live = [e for e in self.entries.values() if e is not None]
        return (self.table, self.starts, [e.buf for e in live])

    def get(self, desc, mode, wsA, wsB=None):
        """Packed forms for (desc, mode) of the given component tensors, or None if the shape runs on the 16/48-product
        kernels.  Fresh with respect to the weights as they are when the returned launch order is reached."""
        ws = list(wsA) + (list(wsB) if wsB is not None else [])
        key = (bytes(desc), mode, tuple(id(w) for w in ws))
        e = self.entries.get(key, 0)
        if e is None:
            return None
        if e == 0 or self._alive(e) is None:
            npair = 2 if wsB is not None else 1
            n = hcq_pack_floats(desc, mode, npair) if all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                                                          for w in ws) else 0
            if n == 0:
                self.entries[key] = None
                return None
            e = self._Entry()
            e.desc = L.ConvDesc.from_buffer_copy(bytes(desc))
            e.mode, e.npair, e.nA = int(mode), npair, len(wsA)
            e.refs = [weakref.ref(w) for w in ws]
            e.buf = torch.empty(n, device=ws[0].device, dtype=torch.float32)
            self._fill(e, ws)
            self.entries[key] = e
        ptrs = tuple(w.data_ptr() for w in ws)
        if ptrs != e.ptrs:
            self._fill(e, ws)
        self.ensure_packed()
        vers = tuple(w._version for w in ws)
        if e.epoch != self.epoch or (e.vers is not None and e.vers != vers):
            wsA_, wsB_ = ws[:e.nA], (ws[e.nA:] if e.npair == 2 else None)
            hcq_pack(desc, mode, wsA_, wsB_, out=e.buf)
            e.epoch = self.epoch
        e.vers = vers
        return e.buf


hcq_weights = _HcqWeights()
L._reload_hooks.append(hcq_weights.reset)       # the forms are packed for the kernels the switches selected


class _GruWeights:
    """Packed recurrent weights of the GRU layers (seld_gru_pack: W_hh and W_hh^T of every direction as MFMA fragments, b_hh,
    zero-padded to a multiple of 16 hidden units), one buffer per layer.  Rebuilt by the rules of the fast-product forms
    above, whose epoch counter it shares: `hcq_weights.weights_changed()` re-packs at the layer's next request (in a
    recorded step that request, and so the pack launch, is part of the graph), an in-place edit torch knows about shows in
    the version counters, a move in the pointers.  Entries hold weak references; dead ones go when a layer registers."""

    class _Entry:
        __slots__ = ("refs", "buf", "ptrs", "vers", "epoch")

    def __init__(self):
        self.entries = {}

    def reset(self):
        self.entries.clear()

    def get(self, hidden, w_hh, b_hh):
        """The packed buffer for `w_hh` (one (3H, H) tensor per direction) and `b_hh` (one (3H,) tensor per direction, or
        all None), fresh with respect to the weights as they are when the returned launch order is reached."""
        dirs = len(w_hh)
        ts = list(w_hh) + [b for b in b_hh if b is not None]
        if len(ts) not in (dirs, 2 * dirs) or any(_req(t, "gru weight") is not t for t in ts):
            raise L.SeldHipError("gru: the recurrent weights must be contiguous, and the biases given for every direction or none")
        key = tuple(id(t) for t in ts)
        e = self.entries.get(key)
        if e is None or any(r() is not t for r, t in zip(e.refs, ts)):
            for k in [k for k, old in self.entries.items() if any(r() is None for r in old.refs)]:
                del self.entries[k]
            e = self._Entry()
            e.refs = [weakref.ref(t) for t in ts]
            e.buf = torch.empty(int(L.lib().seld_gru_pack_floats(dirs, hidden)), device=ts[0].device, dtype=torch.float32)
            e.ptrs = e.vers = None
            e.epoch = -1
            self.entries[key] = e
        ptrs, vers = tuple(t.data_ptr() for t in ts), tuple(t._version for t in ts)
        if e.ptrs != ptrs or e.vers != vers or e.epoch != hcq_weights.epoch:
            L.check(L.lib().seld_gru_pack(dirs, hidden, L.ptr(w_hh[0]), L.ptr(w_hh[-1] if dirs == 2 else None),
                                          L.ptr(b_hh[0]), L.ptr(b_hh[-1] if dirs == 2 else None), L.ptr(e.buf),
                                          L.current_stream()), "seld_gru_pack")
            e.ptrs, e.vers, e.epoch = ptrs, vers, hcq_weights.epoch
        return e.buf


gru_weights = _GruWeights()
