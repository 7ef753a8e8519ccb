"""The recurrent context network (CPCAR: GRU, LSTM, RNN) against the fp64 oracle where real runs go and the rest of the suite
does not look: the carried state (h0 in, h_last out -- what buildFeature and the ABX command line stream every file through,
chunk after chunk) on every form of the cooperative kernels; the streaming kernels at the widths the product trains at (what
takes over past the cooperative window limit, after a cooperative time-out, and for the whole process under the reference's
DDP wrapping on RCCL); and the shapes the streaming kernels accept but nothing else runs (hidden sizes that leave idle lanes,
1024 threads, uneven K slices, an input width other than the hidden size, up to 8 layers).

Every case checks the output, the final state, the input gradient and every parameter gradient, and asserts through
cpc_coop_launches() which kernel family ran."""
import pytest
import torch

import cpc2_amd
from cpc2_amd import _lib
from oracle import cpc_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREFIX = "gAR.baseNet."
_MODES = {"GRU": (synth.gru_params, O.gru_forward), "LSTM": (synth.lstm_params, O.lstm_forward),
          "RNN": (synth.rnn_params, O.rnn_forward)}


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def assert_close(got, ref, tol, what="", rtol=None):
    """(tests/test_gpu_parity.py) max-norm check |got - ref|_inf <= tol * |ref|_inf AND, element by element,
    |got - ref| <= atol + rtol * |ref| with atol = tol * |ref|_inf and rtol = 64 * tol by default."""
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    atol = tol * float(r.abs().max()) + 1e-30
    rt = 64 * tol if rtol is None else rtol
    bad = (g - r).abs() > atol + rt * r.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside atol {atol:.2e} + {rt:.1e} |ref|"


# ----------------------------------------------------------------------------- policy and kernel selection
def _set_policy(value):
    lib = _lib.load()
    prev = lib.cpc_coop_set_policy(-1)
    lib.cpc_coop_set_policy(value)
    try:
        yield lib
    finally:
        lib.cpc_coop_set_policy(prev)


@pytest.fixture
def default_policy():
    """The cooperative kernels wherever they fit (the policy is process-wide: restored afterwards)."""
    yield from _set_policy(0)


@pytest.fixture
def streaming_only():
    """cpc_coop_set_policy(1): the streaming kernels only, as after a cooperative time-out or under DDP on RCCL."""
    yield from _set_policy(1)


_COOP_MEMBERS = {256: 4, 512: 16}      # workgroups per group of the cooperative kernels (coop.h, CoopCfg<H>::G)


def windows_per_group(hid, n):
    """coop.h coop_windows_per_group: the windows one group of the cooperative kernels takes (0: streaming kernels)."""
    g = _COOP_MEMBERS.get(hid)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    if g is None or n_cus < g:
        return 0
    for nb in (1, 2, 4, 8):
        if -(-n // nb) <= n_cus // g:
            return nb
    return 0


def window_limit(hid):
    """The most windows the cooperative kernels take at once: (CUs / G) groups of 8."""
    return torch.cuda.get_device_properties(0).multi_processor_count // _COOP_MEMBERS[hid] * 8


# ----------------------------------------------------------------------------- one case: HIP module and fp64 oracle
def _case(mode, din, hid, layers, n, t_len, with_h0, seed):
    params = _MODES[mode][0](din, hid, layers, seed)
    x = synth.features((n, t_len, din), seed + 1, relu=True)
    gout = synth.features((n, t_len, hid), seed + 2)
    state = None
    if with_h0:
        h0 = synth.features((layers, n, hid), seed + 3, scale=0.5)
        state = (h0, synth.features((layers, n, hid), seed + 4)) if mode == "LSTM" else (h0,)
    return params, x, gout, state


def _oracle(mode, params, x, gout, state, layers, chunks, reverse=False):
    """fp64: the chunks one after the other, each from the (detached) final state of the one before -- keepHidden's semantics."""
    fwd = _MODES[mode][1]
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(True)
    st = tuple(s.double() for s in state) if state is not None else None
    outs = []
    for a, b in chunks:
        kw = {} if st is None else ({"h0": st[0], "c0": st[1]} if mode == "LSTM" else {"h0": st[0]})
        res = fwd(x64[:, a:b], p64, layers, PREFIX, reverse=reverse, **kw)
        outs.append(res[0])
        st = tuple(r.detach() for r in res[1:])
    out = torch.cat(outs, dim=1)
    (out * gout.double()).sum().backward()
    return out.detach(), st, x64.grad, {k[len("gAR."):]: p.grad for k, p in p64.items()}


def _hip(mode, params, x, gout, state, din, hid, layers, chunks, reverse=False):
    """The public module: keepHidden=True, ar.hidden = the initial state, ar.hidden read back as the final one."""
    lib = _lib.load()
    ar = cpc2_amd.CPCAR(din, hid, True, layers, mode=mode, reverse=reverse)
    ar.load_state_dict({k[len("gAR."):]: v for k, v in params.items()})
    ar = ar.to(DEV)
    if state is not None:
        ar.hidden = tuple(s.to(DEV) for s in state) if mode == "LSTM" else state[0].to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    before = lib.cpc_coop_launches()
    out = torch.cat([ar(xd[:, a:b]) for a, b in chunks], dim=1)
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    launches = lib.cpc_coop_launches() - before
    _lib.check(lib.cpc_async_error_check(_lib.stream_ptr(torch.device(DEV))), "async error check")
    st = ar.hidden if mode == "LSTM" else (ar.hidden,)
    return out.detach(), st, xd.grad, {name: p.grad for name, p in ar.named_parameters()}, launches


def _check(mode, din, hid, layers, n, t_len, with_h0, chunks=None, reverse=False, seed=9, result=None):
    """Runs one case both ways and compares everything; returns the cooperative launches the HIP run made (and, in `result`,
    what the HIP run gave: output and final state)."""
    chunks = chunks or [(0, t_len)]
    params, x, gout, state = _case(mode, din, hid, layers, n, t_len, with_h0, seed)
    ref, ref_st, ref_dx, ref_grads = _oracle(mode, params, x, gout, state, layers, chunks, reverse)
    out, st, dx, grads, launches = _hip(mode, params, x, gout, state, din, hid, layers, chunks, reverse)
    tag = f"{mode} H={hid} in={din} layers={layers} n={n} t={t_len}"
    assert_close(out, ref, 1e-5, f"{tag} out")
    assert st is not None and len(st) == len(ref_st)
    for name, got, want in zip(("h_last", "c_last"), st, ref_st):
        assert tuple(got.shape) == (layers, n, hid), f"{tag} {name} shape {tuple(got.shape)}"
        assert_close(got, want, 1e-5, f"{tag} {name}")
    assert_close(dx, ref_dx, 1e-4, f"{tag} dx")
    assert set(grads) == set(ref_grads)
    for name, g in grads.items():
        assert_close(g, ref_grads[name], 1e-4, f"{tag} grad {name}")
    if result is not None:
        result.update(out=out, state=st)
    return launches


# ----------------------------------------------------------------------------- A. carried state on every cooperative form
# The window counts of test_gru_vs_oracle_fp64: with 256 CUs, H = 256 has 64 groups of 4 workgroups and H = 512 16 groups of
# 16, so nb windows per group cover up to 64 nb and 16 nb windows.  The matrix-pipe forms are the default at H = 512, nb = 8
# (forward and backward) and for the backward at H = 256, nb >= 2 (gru.hip, mfma_wanted); the FMA (VALU) forms everywhere else.
@pytest.mark.parametrize("hid,layers,n,t_len,nb", [
    (256, 1, 5, 16, 1),         # VALU forward and backward
    (256, 1, 128, 5, 2),        # VALU forward, matrix-pipe backward
    (256, 2, 130, 7, 4),        # ... ragged last group (2 of 4 windows), two layers
    (256, 1, 300, 6, 8),        # ... ragged last group (4 of 8)
    (512, 2, 3, 12, 1),         # VALU forward and backward, two layers
    (512, 1, 20, 9, 2),
    (512, 1, 19, 9, 2),         # ragged last group (1 of 2)
    (512, 1, 40, 10, 4),
    (512, 2, 100, 8, 8),        # matrix-pipe forward and backward; ragged last group (4 of 8), two layers
    (512, 1, 65, 3, 8),         # ... ragged last group of ONE window
])
def test_gru_carried_state_on_the_cooperative_kernels(default_policy, hid, layers, n, t_len, nb):
    assert windows_per_group(hid, n) == nb, f"{n} windows at H = {hid} are not {nb} per group on this device"
    launches = _check("GRU", hid, hid, layers, n, t_len, with_h0=True)
    assert launches == 2 * layers, f"{launches} cooperative launches (forward and backward of {layers} layers expected)"


# two chunks: the second starts from the first one's h_last; the whole against the oracle of the whole sequence
@pytest.mark.parametrize("mode,hid,layers,n,t_len", [
    ("GRU", 256, 1, 6, 16), ("GRU", 256, 2, 70, 12),         # VALU forward; VALU / matrix-pipe (nb = 2) backward
    ("GRU", 512, 1, 100, 10), ("GRU", 512, 2, 21, 8),        # matrix-pipe (nb = 8) / VALU (nb = 2) forward and backward
    ("LSTM", 256, 2, 6, 16), ("LSTM", 256, 1, 130, 8), ("LSTM", 512, 1, 21, 10), ("LSTM", 512, 2, 100, 6),
    ("RNN", 256, 2, 6, 16), ("RNN", 512, 1, 21, 10),
])
def test_two_chunks_with_carried_state_equal_the_whole_sequence(default_policy, mode, hid, layers, n, t_len):
    half = t_len // 2
    params, x, gout, state = _case(mode, hid, hid, layers, n, t_len, True, 21)
    ref_whole, ref_whole_st, _dx, _g = _oracle(mode, params, x, gout, state, layers, [(0, t_len)])
    hip = {}
    launches = _check(mode, hid, hid, layers, n, t_len, with_h0=True, chunks=[(0, half), (half, t_len)], seed=21, result=hip)
    assert_close(hip["out"], ref_whole, 1e-5, f"{mode} chunks vs the whole sequence")
    for got, want in zip(hip["state"], ref_whole_st):
        assert_close(got, want, 1e-5, f"{mode} carried state vs the whole sequence")
    # the RNN has no cooperative kernel: every one of its cases runs the streaming kernels
    expected = 0 if mode == "RNN" else 2 * 2 * layers
    assert launches == expected, f"{launches} cooperative launches, {expected} expected"


@pytest.mark.parametrize("mode,hid,layers,n,t_len", [
    ("LSTM", 256, 1, 5, 16), ("LSTM", 256, 1, 70, 6), ("LSTM", 256, 2, 130, 7), ("LSTM", 256, 1, 300, 5),
    ("LSTM", 512, 2, 3, 12), ("LSTM", 512, 1, 19, 9), ("LSTM", 512, 1, 40, 8), ("LSTM", 512, 1, 65, 4),
    ("RNN", 256, 1, 5, 16), ("RNN", 512, 2, 19, 9),
])
def test_lstm_rnn_carried_state(default_policy, mode, hid, layers, n, t_len):
    launches = _check(mode, hid, hid, layers, n, t_len, with_h0=True)
    expected = 0 if mode == "RNN" else 2 * layers
    assert launches == expected, f"{launches} cooperative launches, {expected} expected"


# ----------------------------------------------------------------------------- B. streaming kernels at H = 256 / 512
@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
@pytest.mark.parametrize("hid", [256, 512])
@pytest.mark.parametrize("layers,n,t_len,with_h0,reverse", [
    (1, 1, 1, False, False), (2, 7, 20, True, False), (1, 64, 20, True, False), (2, 64, 1, False, False),
    (1, 7, 1, True, False), (2, 1, 20, False, False), (1, 7, 20, True, True), (2, 64, 20, False, True),
])
def test_streaming_kernels_at_the_trained_widths(streaming_only, mode, hid, layers, n, t_len, with_h0, reverse):
    launches = _check(mode, hid, hid, layers, n, t_len, with_h0, reverse=reverse)
    assert launches == 0, f"{launches} cooperative launches under the streaming-only policy"


@pytest.mark.parametrize("mode", ["GRU", "LSTM"])
@pytest.mark.parametrize("hid", [256, 512])
def test_window_limit_of_the_cooperative_kernels(default_policy, mode, hid):
    """One window past the limit: the streaming kernels; at the limit: the cooperative ones (8 windows per group)."""
    limit = window_limit(hid)
    assert windows_per_group(hid, limit) == 8 and windows_per_group(hid, limit + 1) == 0
    launches = _check(mode, hid, hid, 1, limit + 1, 3, with_h0=True)
    assert launches == 0, f"{launches} cooperative launches at {limit + 1} windows (limit {limit})"
    launches = _check(mode, hid, hid, 1, limit, 3, with_h0=True)
    assert launches == 2, f"{launches} cooperative launches at {limit} windows (forward and backward expected)"


# ----------------------------------------------------------------------------- C. the shapes the streaming kernels accept
# threads per window of the streaming GRU = kq * hp (hp = H rounded up to 64; kq = K slices): H = 4 -> 1 x 64 with 60 idle
# lanes; 36 -> 9 slices of one float4; 100 -> 8 x 128 = 1024 threads, 28 idle lanes; 320 -> 3 uneven slices (27, 27, 26
# float4s); 1020 -> 1 x 1024, 4 idle lanes; 1024 -> 1 x 1024.  The input width changes W_ih^T's transpose and the
# input-gradient scratch (max(in, H)).
@pytest.mark.parametrize("hid,din,layers,n,t_len", [
    (4, 1, 1, 3, 20), (4, 40, 3, 2, 9), (36, 3, 2, 5, 17), (36, 36, 3, 4, 10), (12, 1, 8, 3, 6), (8, 40, 8, 2, 5),
    (100, 40, 1, 6, 12), (100, 200, 2, 3, 7), (320, 640, 1, 4, 9), (320, 1, 1, 1, 1), (1020, 40, 1, 2, 5),
    (1020, 3, 2, 1, 3), (1024, 2048, 1, 2, 4), (1024, 3, 2, 1, 1),
])
def test_gru_streaming_shape_domain(default_policy, hid, din, layers, n, t_len):
    launches = _check("GRU", din, hid, layers, n, t_len, with_h0=True)
    assert launches == 0


@pytest.mark.parametrize("mode", ["LSTM", "RNN"])
@pytest.mark.parametrize("hid,din,layers,n,t_len,with_h0", [
    (1024, 40, 1, 3, 5, True), (1024, 1024, 2, 1, 3, False), (100, 3, 2, 4, 10, True), (320, 640, 1, 2, 6, True),
    (36, 1, 3, 5, 8, True),
])
def test_lstm_rnn_streaming_shape_domain(default_policy, mode, hid, din, layers, n, t_len, with_h0):
    launches = _check(mode, din, hid, layers, n, t_len, with_h0)
    assert launches == 0


@pytest.mark.parametrize("mode", ["GRU", "LSTM", "RNN"])
def test_shapes_outside_the_domain_are_refused(default_policy, mode):
    x = synth.features((2, 3, 8), 1).to(DEV)
    for hid, layers, msg in ((1028, 1, "hidden 1028 must be a multiple of 4 and <= 1024"),
                             (6, 1, "hidden 6 must be a multiple of 4"), (8, 9, "1..8 layers supported")):
        ar = cpc2_amd.CPCAR(8, hid, False, layers, mode=mode).to(DEV)
        with pytest.raises(ValueError, match=msg):
            ar(x)
    # and the library goes on working
    assert _check(mode, 8, 36, 2, 2, 5, with_h0=True) == 0
