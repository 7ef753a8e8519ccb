"""Making the transformer's and the encoder's ReLU decisions unambiguous in fp32 (oracle, test infrastructure only; shared by
tests/test_criterion_pred_gpu.py, tests/test_transformer_dropout_gpu.py, tests/test_transformer_abi_gpu.py and
tests/test_encoder_abi_gpu.py).  Never imported by cpc2_amd/."""
import torch

from . import cpc_oracle as O

RELU_MARGIN = 1e-5


def settle_relu_decisions(p, prefix, c_w, n_classifiers=1, size_seq=None, drop=None):
    """Move every ReLU decision of the transformer's feed-forward net on the input c_w out of reach of fp32 rounding.

    A one-layer predictor at these shapes evaluates 3 * 116 * 2048 pre-activations y lin1^T + b of size O(1); the smallest of
    them in magnitude are ~1e-7 and below, i.e. inside the rounding error of their fp32 evaluation (a 256- or 512-term dot
    product: a few 1e-7).  The kernel may then take relu'(pre) the other way than the fp64 oracle, and the gradients below that
    unit differ by a WHOLE TERM -- measured on the parameters of synth seed 85 at d_model 256: pre = +3.6e-8 at (0, 70, unit
    1466), the kernel's dx differs from the oracle's by 5.7e-3 of its scale at frame (0, 70) alone, and the oracle with that one
    decision flipped reproduces the kernel's dx to 5e-7 -- which says nothing about the arithmetic under test (the encoder's
    tests take the decisions from the kernel for the same reason: oracle.encoder_forward, masks).  Here the parameters are
    made unambiguous instead, judged by the ORACLE's numbers alone: while a pre-activation lies within RELU_MARGIN = 1e-5 of
    zero (30 x the rounding error), lin1.bias of its unit is raised by 3 RELU_MARGIN -- in the fp32 parameters both sides
    load.

    size_seq, drop: as O.transformer_layer_forward takes them (attention dropout changes the pre-activations, so a
    training-mode comparison settles them under the masks it will run with)."""
    bias = p[f"{prefix}ffnetwork.lin1.bias"]
    for _ in range(50):
        pre = []
        with torch.no_grad():
            O.transformer_layer_forward(c_w.double(), {n: v.double() for n, v in p.items() if n.startswith(prefix)}, prefix,
                                        size_seq=size_seq, n_classifiers=n_classifiers, pre_out=pre, drop=drop)
        near = (pre[0].abs() < RELU_MARGIN).reshape(-1, pre[0].shape[-1]).any(dim=0)
        if not bool(near.any()):
            return
        bias[near] += 3 * RELU_MARGIN
    raise AssertionError(f"{prefix}: the ReLU decisions did not settle")


def settle_encoder_relu_decisions(p, prefix, x, margin=RELU_MARGIN):
    """The same for the encoder's five ReLUs on the windows x [N, 1, L], judged by the fp64 numbers alone: while a pre-activation
    relu's argument norm_i(conv_i(.)) lies within `margin` of zero RELATIVE to layer i's largest (they are O(1) after ChannelNorm),
    batchNorm{i}.bias of its channel is raised by 3 margin times that largest -- in the fp32 parameters both sides load.  Layer
    by layer from the input: a layer's bias moves the pre-activations of that layer by a constant per channel and changes nothing
    above it, so one forward pass settles all five.  Returns how many (layer, channel) biases were raised.

    Why not by the choice of seed alone: under synth.encoder_params / synth.audio_windows about 3 in 1e5 pre-activations lie
    within 1e-5 of zero relative to their layer's largest (a density of ~0.4 per unit against a largest of ~4), so a case of
    1e5 pre-activations has a clean seed in a handful of tries, one of 3e6 (one 20480-sample window at hidden 512) never."""
    import torch.nn.functional as F
    raised = 0
    h = x.double()
    with torch.no_grad():
        for i, (_k, s, pad) in enumerate(O.ENCODER_GEOMETRY):
            u = F.conv1d(h, p[f"{prefix}conv{i}.weight"].double(), p[f"{prefix}conv{i}.bias"].double(), stride=s, padding=pad)
            beta = p[f"{prefix}batchNorm{i}.bias"]
            for _ in range(50):
                pre = O.channel_norm(u, p[f"{prefix}batchNorm{i}.weight"].double(), beta.double())
                top = float(pre.abs().max())
                near = (pre.abs() < margin * top).any(dim=2).any(dim=0)
                if not bool(near.any()):
                    break
                beta[0, near, 0] += 3 * margin * top
                raised += int(near.sum())
            else:
                raise AssertionError(f"{prefix}batchNorm{i}: the ReLU decisions did not settle")
            h = torch.relu(pre)
    return raised
