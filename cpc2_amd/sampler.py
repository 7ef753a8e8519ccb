"""The criterion's negative-index sampler (cpc/criterion/criterion.py:247-266).

Negative indices are drawn on the HOST with the same MT19937 stream torch's CPU generator would produce (the reference's CPU
path); by default the sampler consumes -- and advances -- torch's global CPU generator, so `torch.manual_seed(s)` gives
bit-identical indices to the reference.  The library draws the next call's words ahead on a worker thread and keeps the
generator right whatever becomes of that draw (cpc2_hip.h: cpc_negidx_draw_ahead / cpc_negidx_take); this module decides which
buffers a call is served from.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr


def _sleep_until(event):
    """Wait for a device event WITHOUT spinning on a core: this is where the training thread stands still while it is its two steps
    ahead of the device (2.4-2.8 ms of every 4.8 ms step), and hipEventSynchronize -- blocking-sync flag or not -- burns that time
    as CPU time (bench.py: host.thread_cpu_ms_per_step 4.1 against 1.4 of work); eight ranks share one host."""
    import time
    while not event.query():
        time.sleep(0.0001)


class NegativeSampler:
    """Host MT19937 sampler (cpc_negidx_sample_host) + pinned staging ring for the H2D copy."""

    RING = int(os.environ.get("CPC_SAMPLER_RING", "4"))

    def __init__(self):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p(self._lib.cpc_mt_create(5489))
        if not self._h:
            raise MemoryError("cpc_mt_create failed")
        self.follow_torch = True      # consume torch's global CPU generator (reference semantics)
        self._ring, self._dev_ring, self._ext_ring, self._events, self._slot = {}, {}, {}, {}, 0
        self._prefetched = None       # (key, slot, shape) of the draw ahead, or None.  Forgetting it is all it takes to drop one:
        #                               the library's next synchronous call puts the generator where it belongs
        self._torch_seen = None       # follow_torch: torch's generator state as this sampler last left it
        self._ahead_shape = None      # (n, device, shape) the draws ahead are made for: the largest call seen
        self._ahead_misses = 0        # calls in a row that were not the one drawn for
        self._last = None             # (key, slot) of the previous device-side call: its buffers' release event is recorded by the next one
        # draw the next call's words during this step, on a worker thread with a stream of its own.  On by default since round 6: a
        # draw ahead that turns out not to fit (another size, a host-side call, torch's generator used by someone else) is undone,
        # so the index sequence is the reference's either way (tests: test_prefetch_*); False = everything at call time
        self.prefetch = True
        self.alias_ring = False       # opt-in with prefetch: sample() returns one of RING persistent buffers instead of a copy of it
        self.served = collections.Counter()   # sample(time_major=True) calls by the way they were served: "ahead", "prefix", "drawn"

    def __del__(self):
        try:
            if self._h:
                self._lib.cpc_mt_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def seed(self, seed):
        """Private stream seeded like torch.manual_seed(seed); stops following the global generator."""
        check(self._lib.cpc_mt_seed(self._h, ctypes.c_uint32(int(seed) & 0xFFFFFFFF)), "mt_seed")
        self.follow_torch = False
        self._prefetched = None

    # torch CPU generator legacy state: u64 seed, i32 left, i32 seeded, u64 next, u64 mt[624], ...
    def _pull_torch_state(self):
        st = torch.get_rng_state().numpy()
        left = int(st[8:12].view(np.int32)[0])
        nxt = int(st[16:24].view(np.uint64)[0])
        mt = np.ascontiguousarray(st[24:24 + 624 * 8].view(np.uint64).astype(np.uint32))
        check(self._lib.cpc_mt_set_state(self._h, mt.ctypes.data_as(ctypes.c_void_p), left, nxt), "mt_set_state")
        return st

    def _push_torch_state(self, st):
        mt = np.empty(624, dtype=np.uint32)
        left, nxt = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.cpc_mt_get_state(self._h, mt.ctypes.data_as(ctypes.c_void_p), ctypes.byref(left),
                                         ctypes.byref(nxt)), "mt_get_state")
        st = st.copy()
        st[8:12].view(np.int32)[0] = left.value
        st[16:24].view(np.uint64)[0] = nxt.value
        st[24:24 + 624 * 8].view(np.uint64)[:] = mt.astype(np.uint64)
        torch.set_rng_state(torch.from_numpy(st))
        self._torch_seen = st[8:24 + 624 * 8].copy()      # what torch's generator holds after this sampler's draw

    def _torch_unchanged(self):
        """Has nobody drawn from torch's global CPU generator since this sampler left it (a draw ahead is only valid then)?"""
        if self._torch_seen is None:
            return False
        return np.array_equal(torch.get_rng_state().numpy()[8:24 + 624 * 8], self._torch_seen)

    def sample_host(self, batch, seq_len, window, n_neg, out=None, want_parts=False, time_major=False):
        """int32 extIdx on the host (criterion.py:247-266): [batch, n_neg, window] in the reference's
        order, or the same values as [batch, window, n_neg] with time_major (the kernels' layout)."""
        n = batch * n_neg * window
        self._prefetched = None
        if out is None:
            out = torch.empty(n, dtype=torch.int32)
        bidx = torch.empty(n, dtype=torch.int64) if want_parts else None
        sidx = torch.empty(n, dtype=torch.int64) if want_parts else None
        st = self._pull_torch_state() if self.follow_torch else None
        check(self._lib.cpc_negidx_sample_host(self._h, batch, seq_len, window, n_neg, int(time_major), ptr(out),
                                               ptr(bidx), ptr(sidx)), "negidx_sample_host")
        if st is not None:
            self._push_torch_state(st)
        return (out, bidx, sidx) if want_parts else out

    def _rings(self, key, n, device):
        if key not in self._ring:
            self._ring[key] = [torch.empty(2 * n, dtype=torch.int32).pin_memory() for _ in range(self.RING)]
            self._dev_ring[key] = [torch.empty(2 * n, dtype=torch.int32, device=device) for _ in range(self.RING)]
            self._ext_ring[key] = [torch.empty(n, dtype=torch.int32, device=device) for _ in range(self.RING)]
            self._events[key] = [None] * self.RING
        return self._ring[key], self._dev_ring[key], self._events[key]

    def _next_slot(self, events):
        """The ring slot to fill next, once the kernel that last read its buffers has finished."""
        slot = self._slot % self.RING
        self._slot += 1
        if events[slot] is not None:
            with _lib.host_wait("sampler_buffer_event"):
                _sleep_until(events[slot])
        return slot

    def _take(self, n, device):
        """This call uses the first 2 n of the words drawn ahead: waits for the worker's HOST part -- the draw, the enqueue of copy +
        expansion on its stream -- and orders the training stream behind the event recorded there (the host is not held up by the
        device)."""
        with _lib.host_wait("sampler_worker"):
            check(self._lib.cpc_negidx_take(self._h, 2 * n, _lib.stream_ptr(device)), "negidx_take")

    def _expand(self, raw, shape, device):
        batch, seq_len, window, n_neg = shape
        ext = torch.empty(batch * n_neg * window, dtype=torch.int32, device=device)
        check(self._lib.cpc_negidx_expand(ptr(raw), ptr(ext), batch, seq_len, window, n_neg, _lib.stream_ptr(device)), "negidx_expand")
        return ext

    def sample(self, batch, seq_len, window, n_neg, device, time_major=True):
        """Device int32 extIdx.  time_major (the fused kernels' layout): the host only draws the raw MT19937
        words into a pinned buffer (with `prefetch`: on a worker thread, one call ahead), the device does the
        integer arithmetic (cpc_negidx_expand).  Otherwise: full host path, reference order.

        A draw ahead is made for the LARGEST call seen so far (the full batch).  The stream of words is one sequence whatever it is
        cut into -- a call of n negatives consumes its first 2 n -- so a call is served in one of three ways (counted in `served`):
          * "ahead": it is the call the draw ahead was made for (under follow_torch: and nobody else used torch's generator in
            between): indices already expanded by the worker, nothing on the caller's stream but a wait;
          * "prefix": a SMALLER call on the same device, private stream only, fewer than 8 misses in a row (the same-speaker sampler
            ends every speaker with a partial batch): its 2 n words are a prefix of the words already on the device, one expansion
            kernel;
          * "drawn": anything else (no draw ahead, a larger call, another device, torch's generator): the call draws for itself.
        The library puts the generator behind the words a call took, or back in front of a draw nobody took, so the index
        sequence is the reference's either way (tests: test_prefetch_*)."""
        n = batch * n_neg * window
        if not time_major:
            host = self.sample_host(batch, seq_len, window, n_neg)
            return host.to(device)
        device = torch.device(device)
        key = (n, str(device))
        shape = (batch, seq_len, window, n_neg)
        # The buffers of the PREVIOUS call's slot are free again once everything enqueued since -- that call's expansion and the
        # criterion kernels that read its index tensor -- has run: marked here, one call later, on the stream those kernels are on.
        if self._last is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            self._events[self._last[0]][self._last[1]] = ev
        ahead, self._prefetched = self._prefetched, None        # (key, slot, shape) of the draw ahead, or None
        if ahead is not None and self.follow_torch and not self._torch_unchanged():
            ahead = None                                # someone else drew from torch's generator meanwhile: ITS state decides
        if ahead is not None and ahead[0] == key:
            how, ext = "ahead", self._serve_ahead(ahead, shape, device)
        elif ahead is not None and not self.follow_torch and n < ahead[0][0] and ahead[0][1] == key[1] and self._ahead_misses < 8:
            how, ext = "prefix", self._serve_prefix(ahead, shape, device)
        else:
            how, ext = "drawn", self._serve_drawn(key, shape, device)
        self.served[how] += 1
        if self.prefetch:
            self._draw_ahead(n, shape, device)
        return ext

    def _serve_ahead(self, ahead, shape, device):
        """The call the draw was made for: drawn, uploaded AND expanded (on the worker's own stream) while the GPU was busy."""
        akey, aslot, ashape = ahead
        self._take(akey[0], device)
        if ashape == shape:
            # (a COPY of the ring buffer, 3.8 MB at the benchmark shape: the worker rewrites the buffer RING - 1 calls later, and
            #  a caller may keep the indices -- saved for a backward that runs late, logged, compared -- for longer than that;
            #  `alias_ring = True` hands out the buffer itself to a caller that consumes it before the next RING - 1 samples)
            ext = self._ext_ring[akey][aslot] if self.alias_ring else self._ext_ring[akey][aslot].clone()
        else:                              # (the same number of words for another shape: the words are right, the expansion is not)
            ext = self._expand(self._dev_ring[akey][aslot], shape, device)
        self._last = (akey, aslot)
        self._ahead_misses = 0
        if self.follow_torch:              # torch's generator moves on by what the reference's two randint calls consume
            self._push_torch_state(torch.get_rng_state().numpy())
        return ext

    def _serve_prefix(self, ahead, shape, device):
        """A smaller call: its words are the first 2 n of those already on the device.  (Bounded: after eight calls in a row that
        were not the one drawn for, the draws ahead follow the calls' new size instead.)"""
        akey, aslot, _ashape = ahead
        self._take(shape[0] * shape[3] * shape[2], device)
        self._last = (akey, aslot)
        self._ahead_misses += 1
        return self._expand(self._dev_ring[akey][aslot], shape, device)

    def _serve_drawn(self, key, shape, device):
        """The call draws for itself, into a ring of its own size: exactly the words the reference's two torch.randint calls would
        consume (criterion.py:247-256)."""
        ring, dev_ring, events = self._rings(key, key[0], device)
        slot = self._next_slot(events)
        st = self._pull_torch_state() if self.follow_torch else None
        check(self._lib.cpc_mt_draw_host(self._h, ptr(ring[slot]), 2 * key[0]), "mt_draw_host")
        if st is not None:
            self._push_torch_state(st)
        dev_ring[slot].copy_(ring[slot], non_blocking=True)
        self._last = (key, slot)
        return self._expand(dev_ring[slot], shape, device)

    def _draw_ahead(self, n, shape, device):
        """Draw the NEXT call's words now, on the library's worker thread, for the largest call seen so far."""
        if self._ahead_shape is None or self._ahead_shape[1] != str(device) or n > self._ahead_shape[0] or self._ahead_misses >= 8:
            self._ahead_shape = (n, str(device), shape)
            self._ahead_misses = 0
        an, _adev, ashape = self._ahead_shape
        akey = (an, str(device))
        aring, adev_ring, aevents = self._rings(akey, an, device)
        aslot = self._next_slot(aevents)
        check(self._lib.cpc_negidx_draw_ahead(self._h, ptr(aring[aslot]), ptr(adev_ring[aslot]), ptr(self._ext_ring[akey][aslot]),
                                              _lib.device_index(device), *ashape, _lib.stream_ptr(device)), "negidx_draw_ahead")
        self._prefetched = (akey, aslot, ashape)
