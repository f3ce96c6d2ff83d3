"""The flat fp32 gradient buffer behind a module whose parameters are views of one flat buffer, and the rule for what it holds:

    the gradient of a tensor = the sum over the backwards since zero_grad() in which it was trainable;
    a range no backward wrote holds zeros; a frozen tensor's .grad stays None (unless the user left one there), as torch leaves it.

The engine writes a trainable tensor's range (accumulate = 0) or adds to it (accumulate = 1) and leaves frozen ranges alone, so the
ledger zeroes what would otherwise keep stale values: a tensor that turns trainable inside an accumulation window starts from zero, a
tensor frozen since the last window loses its stale values and its .grad view. Plain torch, no native library: tests/test_grad_ledger.py
drives it on the CPU with a stand-in engine."""
import math

import torch


def flat_view(flat, off, shape):
    """flat[off : off + prod(shape)] as a tensor of `shape`. A 4-d shape is a conv weight: logical OIHW with channels_last strides ==
    the physical OHWI image the kernels read."""
    v = flat[off:off + math.prod(shape)]
    if len(shape) == 4:
        O, I, kh, kw = shape
        return v.view(O, kh, kw, I).permute(0, 3, 1, 2)
    return v.view(shape)


def _spans(ranges, idx):
    """[(begin, end)] covering the ranges idx (ascending), neighbours merged: one fill each"""
    out = []
    for i in idx:
        off, n = ranges[i]
        if out and out[-1][1] == off:
            out[-1] = (out[-1][0], off + n)
        else:
            out.append((off, off + n))
    return out


class GradLedger:
    def __init__(self, ranges):
        """ranges: [(offset, count)] of every parameter tensor in the flat buffers, ascending and gap-free. The per-tensor lists below
        and every `params` / `req` argument follow that order."""
        self.ranges = ranges
        self.buffer = None                       # created by grads(); None until somebody asks for it
        self.fresh = True                        # no backward since zero_grad(): the next one overwrites instead of accumulating
        self.written = [False] * len(ranges)     # a backward wrote this tensor's gradient since zero_grad()
        self.dirty = [False] * len(ranges)       # its range of the buffer may hold something other than zeros
        self.viewed = [False] * len(ranges)      # grads() has given this tensor its .grad view

    def drop(self):
        """forget the buffer (re-flatten, copies): nothing written, nothing to accumulate onto. The caller clears the .grad views."""
        self.__init__(self.ranges)

    def pending(self):
        """gradients of a backward since zero_grad() are in the buffer"""
        return self.buffer is not None and not self.fresh

    def grads(self, flat_params, params):
        """The buffer (zeros_like(flat_params) on first use). `.grad` views into it are attached to the tensors that require grad
        (whoever fills the buffer by hand sees the values through them) or whose gradient a backward has written since zero_grad().
        params: callable returning the parameter tensors, asked only while some tensor has no view yet."""
        if self.buffer is None:
            self.buffer = torch.zeros_like(flat_params)
        if not all(self.viewed):
            self._attach(params())
        return self.buffer

    def _attach(self, params):
        for i, (t, (off, _)) in enumerate(zip(params, self.ranges)):
            if not self.viewed[i] and (self.written[i] or t.requires_grad):
                if t.grad is None:
                    t.grad = flat_view(self.buffer, off, t.shape)
                self.viewed[i] = True

    def begin(self, params, req):
        """Before a backward that writes the gradients of the tensors with req[i] (their requires_grad) into the buffer grads()
        returned: zero the ranges the rule wants zeroed, mark what the backward writes. Returns the engine's accumulate flag."""
        fresh, written, dirty, viewed = self.fresh, self.written, self.dirty, self.viewed
        if fresh:
            stale = [i for i, r in enumerate(req) if not r and dirty[i]]
            for i, r in enumerate(req):
                if r or not (dirty[i] or viewed[i]):
                    continue
                dirty[i] = False
                g = params[i].grad                   # frozen now: its view of the buffer goes, a .grad the user put there stays
                if g is not None and g.device == self.buffer.device and g.data_ptr() == self.buffer.data_ptr() + self.ranges[i][0] * 4:
                    params[i].grad = None
                viewed[i] = False
        else:
            stale = [i for i, r in enumerate(req) if r and not written[i] and dirty[i]]
        for a, b in _spans(self.ranges, stale):
            self.buffer[a:b].zero_()
        for i, r in enumerate(req):
            if r:
                written[i] = dirty[i] = True
        self._attach(params)                         # .grad views for the tensors this backward writes first
        return 0 if fresh else 1

    def finish(self):
        """a backward has written into the buffer: the next one accumulates"""
        self.fresh = False

    def mark_stale(self):
        """zero_grad(): the next backward overwrites instead of accumulating, and until one arrives no tensor has a gradient"""
        self.fresh = True
        self.written = [False] * len(self.ranges)

    def mark_all_written(self):
        """as after a backward with everything trainable (callers that fill the buffer by hand)"""
        self.written = [True] * len(self.ranges)
