"""What `score.Scorer` and `adapt.Adapter` share: an fp64 accumulator tensor on the handle's GPU fed by one read-only kernel in front of
a tag tick (csrc/ekf_pregate.hpp: load_tag_tick), per tick from device tensors or per `DeviceSequence` in one native call."""
import ctypes as C

from . import _tensors as _t
from . import gate as _gate
from .sequence import DeviceSequence


class TagTickObserver:
    """A subclass names its library (LIB, a `SideLibrary`), the planes of its accumulator array (WORDS), what a multirate handle is
    refused as (WHAT), the class `result` reads the accumulators as (RESULT) and whether the multirate refusal is repeated in front of
    every native call (RECHECK) or holds from construction; and makes the one native call of `observe` and of `run`."""
    LIB = WORDS = WHAT = RESULT = None
    RECHECK = False

    def __init__(self, io):
        _gate.refuse_multirate(io.ekf.params, self.WHAT)
        self.io = io
        self._Bp = -(-self.io.ekf.batch // 64) * 64
        self.acc = _t.empty(self.io.ekf.device, (self.WORDS, self._Bp), "float64", zero=True)

    def reset(self):
        self.acc.zero_()

    def _recheck(self):
        if self.RECHECK:
            _gate.refuse_multirate(self.io.ekf.params, self.WHAT)

    def observe(self, u, z, mask=None):
        io = self.io
        B = io.ekf.batch
        src = io._check(u, "u", (B, 6))
        if io._check(z, "z", (B, 7)) != src:
            raise ValueError("u and z must have the same dtype")
        io._check_mask(mask)
        self._recheck()
        D, Q = _t.devio_lib(), self.LIB.load()
        view = io._view()
        iv = io._inputs_view(1)
        with io._ordered(view, u, z, mask, self.acc):
            _t.dcheck(D.qdv_pack_inputs(C.byref(view), C.byref(iv), u.data_ptr(), z.data_ptr(), None if mask is None else mask.data_ptr(),
                                        _t.FLOATS[src]))
            self.LIB.check(self._observe_tick(Q, view, iv))

    def run(self, seq, t0=0, n=None):
        io = self.io
        t0, n = DeviceSequence.window(io, seq, t0, n)
        self._recheck()
        Q = self.LIB.load()
        view = io._view()
        with io._ordered(view, self.acc):
            self.LIB.check(self._run(Q, seq, t0, n))

    def result(self):
        return self.RESULT(self.acc[:, :self.io.ekf.batch])
