"""Shared cases of the learn_3d=True autoencoder tests (tests/test_ae3d_host.py, tests/test_hip_ae3d.py) and of the fixture generator
(tests/golden/make_ae3d_golden.py): configurations, seeded inputs, and plain-torch restatements - the temporal attention on token
rows, the temporal convolution and the whole Factorized3DConvAttn block (ref/models/submodules.py:9-95, 182-255) as functions of a
parameter dict, in whatever dtype the dict has (float64 in the tests).  Every restatement takes `wrong=`: one deliberate mistake,
which the host tests show the fixtures reject."""
import torch
import torch.nn.functional as F

from oracle import ops as O

AE_SMALL = dict(ngf=32, n_downsampling=1, num_res_blocks=1, out_layer='Tanh', learn_3d=True)        # C = 64: A = 8, V = 32
AE64_3D = dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=True)         # the KTH dict with the flag on
PAIR_FRAMES = (2, 3, 1, 8, 8)                                                                        # (N, T, ch, S, S) of ae3d_pair.npz
BLOCK_C = 64
BLOCK_CASES = [(2, 3, 4, 4), (2, 5, 3, 5)]                                                           # (N, T, H, W)
DIMS = [(8, 32), (16, 64), (32, 128), (64, 256)]
# parameters whose exact gradient is 0 in train mode: the four of tests/test_hip_ae_train.py and their temporal counterparts (a conv
# bias before a training BatchNorm; the key bias, which the softmax removes; value and out_proj bias, constants before attn1d's BatchNorm)
ZERO_GRAD = ("spatial_conv.0.bias", "attn2d.Wk.bias", "attn2d.Wv.bias", "attn2d.out_proj.bias",
             "temporal_conv.0.bias", "attn1d.Wk.bias", "attn1d.Wv.bias", "attn1d.out_proj.bias")
WRONG = ("scaled", "softmax_query", "across_pixels", "swap_t_hw", "taps_reversed", "pad_leak", "biased_var", "bn_per_frame",
         "gamma_before_act", "no_skip")


def block_tag(N, T, H, W, conv_first):
    return f"n{N}t{T}h{H}w{W}_{'conv' if conv_first else 'attn'}"


def block_file(N, T, H, W):
    """fixture of a block case (both orders): tests/golden/<name>.npz, one file per grid"""
    return "ae3d_block" if (H, W) == (4, 4) else f"ae3d_block_{H}x{W}"


def block_input(N, T, H, W, seed=300):
    """(x, cotangent) of a block case, (N*T, C, H, W)"""
    shape = (N * T, BLOCK_C, H, W)
    return O.seeded_randn(shape, seed + H * W + T), O.seeded_randn(shape, seed + 50 + H * W + T)


def pair_frames(seed=400):
    return torch.tanh(O.seeded_randn(PAIR_FRAMES, seed))


# ------------------------------------------------------------------------------------------------------------- the kernel's problem
def temporal_attn_ref(q, k, v, N, T, HW, wrong=None):
    """q, k [N*T*HW, A], v [N*T*HW, V] on token rows, row = (n T + t) HW + p  ->  softmax(q k^T) v over the T frames of each pixel,
    [N*T*HW, V]; scores NOT scaled (ref/models/submodules.py:229-237)"""
    def split(t):          # -> (N, HW, T, d): the sequences the attention runs over
        if wrong == "swap_t_hw":
            return t.reshape(N, HW, T, -1)
        if wrong == "across_pixels":
            return t.reshape(N, T, HW, -1)
        return t.reshape(N, T, HW, -1).transpose(1, 2)
    qs, ks, vs = split(q), split(k), split(v)
    s = qs @ ks.transpose(-1, -2)
    if wrong == "scaled":
        s = s * q.shape[-1] ** -0.5
    o = torch.softmax(s, dim=-2 if wrong == "softmax_query" else -1) @ vs
    if wrong in ("swap_t_hw", "across_pixels"):
        return o.reshape(N * T * HW, -1)
    return o.transpose(1, 2).reshape(N * T * HW, -1)


def kernel_inputs(A, V, N, T, HW, seed=500):
    """q (scaled by 1.5 / sqrt(A), as the 2-D kernel's test inputs), k, v and the output cotangent, on token rows"""
    R = N * T * HW
    q = O.seeded_randn((R, A), seed) * (1.5 / A ** 0.5)
    return q, O.seeded_randn((R, A), seed + 1), O.seeded_randn((R, V), seed + 2), O.seeded_randn((R, V), seed + 3)


def temporal_attn_ref64(q, k, v, go, N, T, HW):
    """float64: (o, dq, dk, dv)"""
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    o = temporal_attn_ref(qd, kd, vd, N, T, HW)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


# ------------------------------------------------------------------------------------------------------------------ the block
def _rows(x):
    NT, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(NT * H * W, C)


def _frames(rows, shape):
    NT, C, H, W = shape
    return rows.reshape(NT, H, W, C).permute(0, 3, 1, 2)


def _bn(x, p, pre, train, stats, groups=None, wrong=None):
    """BatchNorm over the rows of x [R, C] with the parameters p[pre + ...]; groups (bn_per_frame): statistics per group of rows"""
    w, b, rm, rv = p[pre + "weight"], p[pre + "bias"], p[pre + "running_mean"], p[pre + "running_var"]
    if not train:
        return (x - rm) / torch.sqrt(rv + 1e-5) * w + b
    if groups is not None:
        xs = x.reshape(groups[0], groups[1], groups[2], -1)            # (N, T, HW, C): per frame t
        mean, var = xs.mean((0, 2), keepdim=True), xs.var((0, 2), unbiased=False, keepdim=True)
        y = ((xs - mean) / torch.sqrt(var + 1e-5)).reshape(x.shape) * w + b
        mean, var, n = mean.mean((0, 1, 2)), var.mean((0, 1, 2)), groups[0] * groups[2]
    else:
        mean, var, n = x.mean(0), x.var(0, unbiased=False), x.shape[0]
        y = (x - mean) / torch.sqrt(var + 1e-5) * w + b
    unb = 1.0 if wrong == "biased_var" else n / (n - 1)
    stats[pre + "running_mean"] = (0.9 * rm + 0.1 * mean).detach()
    stats[pre + "running_var"] = (0.9 * rv + 0.1 * var * unb).detach()
    return y


def _lin(x, p, pre):
    return x @ p[pre + "weight"].t() + p[pre + "bias"]


def _attn2d_ref(x, p, train, stats):
    """NonLocalAttenion2D (ref/models/submodules.py:138-168) on frames x (F, C, H, W)"""
    Fr, C, H, W = x.shape
    tok = _rows(x)
    q = _lin(tok, p, "attn2d.Wq.").reshape(Fr, H * W, -1)
    pool = lambda t: F.max_pool2d(t.reshape(Fr, H, W, -1).permute(0, 3, 1, 2), 2, 2).flatten(2)          # (F, d, HW/4)
    k, v = pool(_lin(tok, p, "attn2d.Wk.")), pool(_lin(tok, p, "attn2d.Wv."))
    o = (torch.softmax(q @ k, -1) @ v.transpose(1, 2)).reshape(Fr * H * W, -1)
    h = torch.relu(_bn(_lin(o, p, "attn2d.out_proj."), p, "attn2d.norm_func.", train, stats))
    return x + p["attn2d.gamma"] * _frames(h, x.shape)


def temporal_conv_ref(rows, w, b, N, T, HW, wrong=None):
    """Conv1d(C, C, 3, padding='same') over the T frames of every pixel, on token rows [N*T*HW, C]; w [C, C, 3]"""
    if wrong == "taps_reversed":
        w = w.flip(-1)
    x = rows.reshape(1, N * T, HW, -1) if wrong == "pad_leak" else rows.reshape(N, T, HW, -1)
    L = x.shape[1]
    xp = F.pad(x, (0, 0, 0, 0, 1, 1))
    y = sum(xp[:, d:d + L] @ w[:, :, d].t() for d in range(3)) + b
    return y.reshape(rows.shape[0], -1)


def block_ref(p, x, T, conv_first, train=True, wrong=None):
    """Factorized3DConvAttn(C, learn_3d=True).forward(x, T) (ref/models/submodules.py:48-95) from the parameter dict p (the block's
    state-dict keys); -> (y, stats): stats holds the updated running statistics (p itself is not changed)"""
    NT, C, H, W = x.shape
    N, HW = NT // T, H * W
    stats = {}
    aw = wrong if wrong in ("scaled", "softmax_query", "across_pixels", "swap_t_hw") else None
    cw = wrong if wrong in ("taps_reversed", "pad_leak") else None
    per_frame = (N, T, HW) if wrong == "bn_per_frame" else None

    def conv2d(y):
        c = F.conv2d(y, p["spatial_conv.0.weight"], p["spatial_conv.0.bias"], padding=1)
        return _frames(torch.relu(_bn(_rows(c), p, "spatial_conv.1.", train, stats)), y.shape) + y

    def conv1d(rows):
        c = temporal_conv_ref(rows, p["temporal_conv.0.weight"], p["temporal_conv.0.bias"], N, T, HW, cw)
        h = torch.relu(_bn(c, p, "temporal_conv.1.", train, stats, per_frame, wrong))
        return h if wrong == "no_skip" else h + rows

    def attn1d(rows):
        o = temporal_attn_ref(_lin(rows, p, "attn1d.Wq."), _lin(rows, p, "attn1d.Wk."), _lin(rows, p, "attn1d.Wv."), N, T, HW, aw)
        h = _bn(_lin(o, p, "attn1d.out_proj."), p, "attn1d.norm_func.", train, stats, per_frame, wrong)
        if wrong == "gamma_before_act":
            return rows + torch.relu(p["attn1d.gamma"] * h)
        return rows + p["attn1d.gamma"] * torch.relu(h)

    if conv_first:
        y = _rows(_attn2d_ref(conv2d(x), p, train, stats))
        y = attn1d(conv1d(y))
    else:
        y = _rows(conv2d(_attn2d_ref(x, p, train, stats)))
        y = conv1d(attn1d(y))
    return _frames(y, x.shape) + x, stats


def block_params(block, dtype=torch.float64, grad=True):
    """the block's state dict as a parameter dict of `dtype`; parameters require grad"""
    names = {n for n, _ in block.named_parameters()}
    return {k: (v.detach().to(dtype).clone().requires_grad_() if grad and k in names else v.detach().to(dtype).clone())
            for k, v in block.state_dict().items() if not k.endswith("num_batches_tracked")}


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
