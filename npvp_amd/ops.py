"""torch.autograd glue over the C ABI of libnpvp_hip.so.  PyTorch supplies device memory,
the current HIP stream and the autograd graph; every piece of arithmetic on the hot path is
a hand-written gfx950 kernel reached through ctypes.  There is no CPU / eager fallback:
tensors must be fp32 CUDA(ROCm) tensors and the library must be built.
"""
import contextlib
import functools
import os
from collections import namedtuple

import torch

from ._lib import lib, check
# scheduling state (per trainer: sched.StepContext) and the process-wide pieces beside it; re-exported here because the rest of the
# package, the tests and the tools reach them as ops.<name>
from . import sched as _S            # (hot paths read the current context as _S._cur.<field>: one global + two attribute loads)
from .sched import (_p, _ptr, _stream, _ws, AmaxSlot, GemmProbe, HbmProbe, ProbeEvent, AuxStream, StepContext, current, use, scoped,
                    remember, rng, GradSink, WgradStream, WgradChain, ReduceQueue, RangeGuard)


def amax_of(t, slot=None):
    """the amax slot of a 2-D fp32 matrix: the one its producer attached (`t._npvp_amax`), else a fresh slot filled by
    the stand-alone reduction kernel (one read of t)"""
    if slot is not None:
        return slot
    for cand in (t, t._base):               # a view is bounded by the slot of the tensor it is a view of
        tag = getattr(cand, "_npvp_amax", None) if cand is not None else None
        if tag is not None and tag[1] == cand._version:     # (an in-place update after the slot was filled voids it)
            return tag[0]
    s = AmaxSlot.new(t.device)
    t2 = t if t.dim() == 2 else t.reshape(-1, t.shape[-1])
    if t2.stride(1) != 1:
        t2 = t2.contiguous()
    check(lib().npvp_amax(_ptr(t2), t2.shape[0], t2.shape[1], t2.stride(0), _ptr(s), _stream()), "npvp_amax")
    t._npvp_amax = (s, t._version)
    return s


def tag_amax(t, slot):
    """attach a producer-filled slot to the tensor object that carries the values on (also across autograd nodes: the
    engine hands the next node the same Python object unless it had to sum two gradients)"""
    if slot is not None:
        t._npvp_amax = (slot, t._version)
    return t


def _row(t, i):
    """device address of row i of a contiguous fp32 matrix (t[i] without building the view: ~1 000 of them per step)"""
    return t.data_ptr() + 4 * i * t.stride(0)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("npvp_amd ops need tensors on an MI355X device (no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError("npvp_amd ops are fp32")


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------- dropout state
class Drop:
    """A dropout / drop-path site: probability, keying mode (0 element, 1 row group) and salt."""
    __slots__ = ("p", "mode", "g1", "g2", "salt")

    def __init__(self, p=0.0, mode=0, g1=1, g2=1):
        self.p, self.mode, self.g1, self.g2 = float(p), mode, g1, g2
        self.salt = _S._cur.rng.next_salt() if p > 0 else 0

    @property
    def on(self):
        return self.p > 0.0

    @classmethod
    def _like(cls, other, mode, g1, g2):
        """same probability and salt (= same mask stream), other keying geometry"""
        d = cls.__new__(cls)
        d.p, d.mode, d.g1, d.g2, d.salt = other.p, mode, g1, g2, other.salt
        return d


NO_DROP = Drop(0.0)
SkipRoles = namedtuple("SkipRoles", "frames forward dgrad wgrad fused")      # (what `skip_roles`, below, returns)
FrameSkip = namedtuple("FrameSkip", "p salt fps")


class SampleSkip(namedtuple("SampleSkip", "frame forward dgrad wgrad fused")):
    """The samples a node's per-sample DropPath (a row-group Drop) drops, for the launches that leave their work out: built once by the node
    (`of`) and handed down as a default-off keyword.  frame: the (p, salt, frames per sample) of the frame kernels; forward, dgrad, wgrad,
    fused: the site as row groups of one sample's token rows - the skip words of the GEMM entry points - where skip_roles gives that launch
    the spec, else NO_DROP.  The switches are read where the node builds it (forward or backward), not where a deferred weight gradient is flushed."""
    __slots__ = ()

    @classmethod
    def of(cls, roles, drop, rows_per_sample, samples, rows):
        on = drop.on and drop.mode == 1
        rs = Drop._like(drop, 1, rows_per_sample, samples) if (on and rows_per_sample * samples == rows) else NO_DROP     # (they cover the rows once)
        frame = FrameSkip(drop.p, drop.salt, rows_per_sample // 64) if (on and roles.frames) else NO_SKIP.frame          # (a frame: 64 token rows)
        return cls(frame, *(rs if r else NO_DROP for r in roles[1:]))


NO_SKIP = SampleSkip(FrameSkip(0.0, 0, 1), NO_DROP, NO_DROP, NO_DROP, NO_DROP)


class DropRecorder:
    """Test hook: while `sites` is a list, every forward kernel that applies a dropout / drop-path mask appends
    (Drop, kind, count) - kind "elem": one decision per flat element index 0..count-1 (nn.Dropout sites and the
    attention-probability dropout, whose key is the flat index of the [groups, heads, L, S] weights); kind "group": one
    decision per row group 0..count-1 (DropPath).  `mask(site)` replays the site's mask through npvp_drop_apply on ones,
    so a parity test can inject the very masks the kernels drew into the oracle (tests/test_hip_dropout.py)."""
    sites = None

    @classmethod
    def note(cls, drop, kind, count):
        if cls.sites is not None and drop.on:
            cls.sites.append((drop, kind, int(count)))

    @staticmethod
    def mask(site, dev):
        """the site's keep-scale per decision (0 or 1/(1-p)) as a flat tensor, from the current device seed"""
        drop, kind, count = site
        if kind == "elem":
            pad = (-count) % 4
            ones = torch.ones((count + pad) // 4, 4, dtype=torch.float32, device=dev)
            return drop_apply(ones, Drop._like(drop, 0, 1, 1)).reshape(-1)[:count]
        ones = torch.ones(count, 4, dtype=torch.float32, device=dev)          # group g = row g (g1 = 1, g2 = count)
        return drop_apply(ones, Drop._like(drop, 1, 1, count))[:, 0].contiguous()


# GEMM arithmetic (NPVP_GEMM=bf16x6|f32), fp32 accumulation on the matrix cores:
#   bf16x6 (default) every fp32 operand is split into three bf16 terms and the six leading cross products run on
#          v_mfma_f32_32x32x16_bf16: ~2^-23 per product, fp32-grade.  Kernels: gemm_wide_kernel (256-row tiles, weights
#          from pre-split planes: the large forward / dgrad shapes) and gemm_split_db_kernel (128 x 128 tiles: small
#          shapes, weight gradients)
#   f32    exact fp32-input MFMA (v_mfma_f32_32x32x2_f32), 1/16 of the bf16 rate: parity triage
#   bf16x3 two-term split, 3 MFMAs per product, ~2^-16: only ever used for weight gradients, opt-in (NPVP_WGRAD=bf16x3)
#   f16x3  two fp16 terms per operand, 3 MFMAs per product, ~2^-22: fp32-grade at half the matrix work of bf16x6.  Operands
#          are scaled by the power of two of their amax slot (csrc/gemm_f16.hip); taken by the large forward / dgrad shapes
#          (weights as scaled fp16 planes) and the weight gradients, everything else runs as bf16x6
GEMM_MODES = {"f32": 0, "bf16x6": 4, "bf16x6db": 4, "bf16x3": 5, "bf16x3db": 5, "f16x3": 6}
GEMM_PRECISION = GEMM_MODES[os.environ.get("NPVP_GEMM", "f16x3")]


# Arithmetic of the WEIGHT-GRADIENT GEMMs.  Default: the same six-term split as forward / dgrad (fp32-grade, what the
# reference's fp32 wgrad delivers).  NPVP_WGRAD=bf16x3 is an OPT-IN fast mode (two bf16 terms, 3 MFMAs per product, 2^-16
# per product): a weight gradient is a leaf of the backward graph, so its rounding error does not propagate through the
# layers, and the reference's small-N vectors are met (weight-gradient rel-L2 4e-6..7e-6), but there is no full-depth,
# full-batch evidence for it - bench.py never measures it unless asked to, and says so in `dtype` when it does.
WGRAD_PRECISION = {"": None, "bf16x6": None, "same": None, "bf16x3": 5}[os.environ.get("NPVP_WGRAD", "")]


def set_gemm_precision(name):
    global GEMM_PRECISION
    GEMM_PRECISION = GEMM_MODES[name]


# Arithmetic of the forward GEMMs of INFERENCE (opt-in, `eval_arithmetic`): f16x3 is the training arithmetic above; f16x1 multiplies
# the high fp16 terms only - ONE matrix instruction per product, 11 significant bits per operand (2.9e-4 rel-L2 per GEMM against the
# exact product), on the same weight planes and amax slots (precision 7 of npvp_gemm_f32: csrc/gemm_f16.hip).  It exists for the
# sampler, whose S * N clips per call are forward-only work; nothing autograd differentiates ever runs in it.
EVAL_ARITHMETICS = ("f16x3", "f16x1")


def eval_launch_precision(arithmetic, gemm_precision, kernel_id, autograd_off, masked=False):
    """The precision one GEMM launch is made with under eval_arithmetic(arithmetic): 7 (one fp16 term) iff the arithmetic is f16x1,
    the GEMM mode is f16x3 (6), the launch runs on the fp16 forward / dgrad kernels (ids 5 / 7), autograd is off and the launch
    carries no row-group mask or row skip (training features the one-term kernels do not take); else `gemm_precision` unchanged.
    A pure function of its arguments."""
    if arithmetic == "f16x1" and gemm_precision == 6 and kernel_id in (5, 7) and autograd_off and not masked:
        return 7
    return gemm_precision


class eval_arithmetic:
    """with eval_arithmetic("f16x1"): the forward GEMMs launched inside, under no_grad, on the fp16 kernels run in the one-term
    arithmetic (see eval_launch_precision); `switched` counts them.  "f16x3" names what runs anyway: nothing changes.  A launch
    autograd will differentiate (or a backward launch) inside the block is made exactly as outside it.  Blocks nest; the innermost
    one decides.  f16x1 exists beside the f16x3 GEMM mode only: entering it in another mode raises."""
    current = None          # the innermost active block (process-wide, like sched._cur: backward nodes run in a thread of their own)

    def __init__(self, name):
        if name not in EVAL_ARITHMETICS:
            raise ValueError(f"eval_arithmetic: unknown arithmetic {name!r} (one of {', '.join(EVAL_ARITHMETICS)})")
        self.name, self.switched, self._outer = name, 0, None

    def __enter__(self):
        if self.name == "f16x1" and GEMM_PRECISION != 6:
            raise RuntimeError("eval_arithmetic('f16x1') needs the f16x3 GEMM mode (NPVP_GEMM=f16x3): the bf16 and f32 kernels "
                               "have no one-term form")
        self._outer, eval_arithmetic.current = eval_arithmetic.current, self
        return self

    def __exit__(self, *exc):
        eval_arithmetic.current, self._outer = self._outer, None
        return False


def arithmetic_scope(name):
    """the block an entry point's `arithmetic=` argument asks for: None -> nothing at all, a name -> eval_arithmetic(name)"""
    return contextlib.nullcontext() if name is None else eval_arithmetic(name)


class _Function(torch.autograd.Function):
    """autograd.Function whose `apply` notes, while an eval_arithmetic block is active, whether autograd was recording at the call:
    inside `forward` grad mode is always off, for a node that will be differentiated too."""
    _recording = 0          # depth of applies made with grad mode on (nested applies inherit it)

    @classmethod
    def apply(cls, *args):
        if eval_arithmetic.current is None or not (torch.is_grad_enabled() or _Function._recording):
            return super().apply(*args)
        _Function._recording += 1
        try:
            return super().apply(*args)
        finally:
            _Function._recording -= 1


def _autograd_off():
    """no graph is being recorded (grad mode off here AND at the enclosing Function.apply) and no backward pass is running"""
    return not (torch.is_grad_enabled() or _Function._recording or torch._C._current_graph_task_id() != -1)


class WeightPlanes:
    """The pre-split planes of every weight that is a GEMM B operand: F planes for the forward GEMM (B = w as [N][K]), D planes
    for dgrad (B = w as [K][N]).  A weight changes once per optimiser step but is staged by every tile of two GEMMs, so it
    is split ONCE per step, into the exact layout of the GEMM's LDS image - the wide GEMM kernels copy it HBM -> LDS by
    LDS-DMA and spend no VALU or VGPR on it.  Format by GEMM mode: bf16x6 = three bf16 term planes (npvp_split_weight),
    f16x3 = two fp16 planes scaled by the power of two of the weight's amax, which lives in the entry's amax slot
    (npvp_split_weight_f16).
      * A view registers itself on first use (split there and then).
      * `refresh_all()` (FlatAdamW.step, right after the AdamW kernel) re-splits EVERY registered view in one batched call
        per format over a device table - not ~350 small launches per step, and no per-call bookkeeping.
      * An in-place torch update (load_state_dict, a test's fill) is caught by the tensor version counter: that view is
        re-split lazily.
    The cache lives ON the owning tensor object (the Parameter, or the flat parameter buffer it is a view of), never in a
    table keyed by device address alone: a freed weight's address is reused by the next model's weights.  The key holds the
    view's device address too: re-pointing `p.data` (FlatBuffers does) makes a NEW entry, and entries whose storage is no longer
    the owner's are dropped.
    `enabled = False` (tests) makes every GEMM split both operands on the fly (bf16x6 128 x 128 kernel only)."""
    enabled = True
    _owners = []            # weak references to tensors that carry a `_npvp_planes` store
    _tables = None          # [(fmt, device table, amax table or None, [entries])] - rebuilt when `_dirty`
    _group_tensors = {}     # (storage address, fmt, device) -> (entry identities, device table, amax table): see refresh_all
    _dirty = True
    _gen = object()         # identity token of the current generation of entries

    class Entry:
        __slots__ = ("fmt", "version", "planes", "w", "amax", "amax_t", "F", "D")

    @classmethod
    def _owner_died(cls, _ref):
        cls._dirty = True

    @classmethod
    def invalidate(cls, owner=None):
        """the parameters changed under the planes (optimiser step): re-split now - every registered weight, or those that are
        views of `owner` (a trainer's flat parameter buffer: another trainer's planes are still current)"""
        cls.refresh_all(owner)

    @classmethod
    def forget(cls, owner):
        """drop the planes cached on `owner` (FlatBuffers re-points parameter storage: the old planes mirror dead memory)"""
        if owner.__dict__.pop("_npvp_planes", None) is not None:
            cls._dirty = True
            cls._gen = object()         # voids every remembered entry (`_npvp_ent`) at once

    @staticmethod
    def _split(ent):
        w = ent.w
        N, K = w.shape
        F, D = _p(ent.planes[0].data_ptr()), _p(ent.planes[1].data_ptr())
        if ent.fmt == 6:
            check(lib().npvp_split_weight_f16(_ptr(w), w.stride(0), N, K, F, D, _ptr(ent.amax), _stream()), "npvp_split_weight_f16")
        else:
            check(lib().npvp_split_weight(_ptr(w), w.stride(0), N, K, F, D, _stream()), "npvp_split_weight")
        ent.version = w._version

    @classmethod
    def get(cls, w, want):
        """want = 'F' (forward, B = w as [N][K]) or 'D' (dgrad, B = w as [K][N]); returns (planes buffer, amax slot or None)
        or None when this weight has no planes."""
        fmt = GEMM_PRECISION
        # fast path (a Parameter that went through the slow path before: the entry and its address are remembered on the tensor
        # object; ~350 lookups per step)
        hit = w.__dict__.get("_npvp_ent")
        if hit is not None:
            ent = hit[0]
            if ent.fmt == fmt and hit[1] == w.data_ptr() and ent.version == w._version and hit[2] is cls._gen and cls.enabled:
                return (ent.F if want == "F" else ent.D), ent.amax
        if not cls.enabled or fmt not in (4, 6) or w.dim() != 2 or w.shape[0] % 8 or w.shape[1] % 8 or w.stride(1) != 1:
            return None
        owner = w._base if w._base is not None else w
        if not owner.is_leaf and owner.grad_fn is not None:
            return None                     # a temporary (e.g. a permuted conv weight): nothing persistent to cache on
        store = owner.__dict__.get("_npvp_planes")
        if store is None:
            import weakref
            store = owner.__dict__["_npvp_planes"] = {}
            cls._owners.append(weakref.ref(owner, cls._owner_died))
        key = (fmt, w.data_ptr(), tuple(w.shape), w.stride(0))
        ent = store.get(key)
        if ent is None:
            live = owner.untyped_storage().data_ptr()
            for k in [k for k, e in store.items() if e.w.untyped_storage().data_ptr() != live]:
                del store[k]                # entries of a storage this owner no longer has (p.data was re-pointed)
            N, K = w.shape
            ent = cls.Entry()
            ent.fmt, ent.w = fmt, w.detach()
            if fmt == 6:
                ent.planes = torch.empty(2, 2 * N * K, dtype=torch.float16, device=w.device)
                ent.amax_t = torch.zeros(AmaxSlot.FLOATS, dtype=torch.float32, device=w.device)
                ent.amax = AmaxSlot(ent.amax_t.data_ptr(), ent.amax_t)
            else:
                ent.planes = torch.empty(2, 3 * N * K, dtype=torch.bfloat16, device=w.device)
                ent.amax = ent.amax_t = None
            ent.F, ent.D = ent.planes[0], ent.planes[1]
            cls._split(ent)
            store[key] = ent
            cls._dirty = True
        elif ent.version != w._version:
            cls._split(ent)
        if w._base is None and tuple(w.shape) == tuple(ent.w.shape):
            w.__dict__["_npvp_ent"] = (ent, w.data_ptr(), cls._gen)
        return (ent.F if want == "F" else ent.D), ent.amax

    @classmethod
    def _entries(cls):
        live = []
        for ref in cls._owners:
            owner = ref()
            if owner is None:
                continue
            live.append(ref)
            for ent in owner.__dict__.get("_npvp_planes", {}).values():
                yield ent
        cls._owners = live

    @classmethod
    def refresh_if_stale(cls):
        """re-split everything if any registered weight was updated in place behind the planes' back (GraphedTrainStep calls
        this before a replay: the captured step refreshes the planes only after ITS optimiser step)"""
        if any(ent.version != ent.w._version for ent in cls._entries()):
            cls.refresh_all()

    epoch = 0               # bumped whenever the parameters changed under us (caches derived from parameters key on it)

    @classmethod
    def refresh_all(cls, owner=None):
        cls.epoch += 1
        if not cls.enabled:
            return
        if cls._dirty or cls._tables is None:
            owner = None                # (the rebuild below hands every entry a fresh, zeroed amax slot: everything is split again)
            groups = {}
            for ent in cls._entries():
                if ent.w.is_cuda:       # (grouped by STORAGE: the weights of one trainer are views of its flat parameter buffer)
                    groups.setdefault((ent.w.untyped_storage().data_ptr(), ent.fmt, ent.w.device), []).append(ent)
            cls._tables = []
            kept = {}
            for gkey, ents in groups.items():
                own_id, fmt, dev = gkey
                # A group whose entries are the ones it had at the last rebuild KEEPS its device table and its amax slots: the rebuild
                # was caused by something else (another model's weights registered or garbage collected), and a captured HIP graph of
                # this trainer's step has the addresses of both baked in - a fresh pair would leave the graph re-splitting into, and
                # its GEMMs reading scales from, memory that the allocator hands to the next caller (round 6: a replayed step went
                # wrong as soon as anything was allocated and written between two replays).
                ids = tuple(id(e) for e in ents)
                old = cls._group_tensors.get(gkey)
                if old is not None and old[0] == ids and (fmt != 6 or all(e.amax_t is old[2] for e in ents)):
                    table, amax_t = old[1], old[2]
                else:
                    amax_t = None
                    if fmt == 6:             # one contiguous slot table per device: zeroed by ONE memset in the batched call
                        amax_t = torch.zeros(len(ents), AmaxSlot.FLOATS, dtype=torch.float32, device=dev)
                        for i, ent in enumerate(ents):
                            ent.amax_t = amax_t
                            ent.amax.ptr, ent.amax.chunk = amax_t.data_ptr() + AmaxSlot.BYTES * i, amax_t
                    rows = []
                    for ent in ents:
                        N, K = ent.w.shape
                        r = [ent.w.data_ptr(), ent.w.stride(0), N, K, ent.planes[0].data_ptr(), ent.planes[1].data_ptr()]
                        rows.append(r + [ent.amax.ptr, 0] if fmt == 6 else r)
                    table = torch.tensor(rows, dtype=torch.int64).to(dev)
                kept[gkey] = (ids, table, amax_t)
                cls._tables.append((fmt, table, amax_t, ents, own_id))
            cls._group_tensors = kept
            cls._dirty = False
        only = None if owner is None else owner.untyped_storage().data_ptr()
        for fmt, table, amax_t, ents, own_id in cls._tables:
            if only is not None and own_id != only:
                continue
            with torch.cuda.device(table.device):
                if fmt == 6:
                    check(lib().npvp_split_weights_f16(_p(table.data_ptr()), table.shape[0], _p(amax_t.data_ptr()),
                                                       amax_t.numel() * 4, _stream()), "npvp_split_weights_f16")
                else:
                    check(lib().npvp_split_weights_batched(_p(table.data_ptr()), table.shape[0], _stream()), "npvp_split_weights_batched")
            for ent in ents:
                ent.version = ent.w._version


# --------------------------------------------------------------------------- raw kernel wrappers


def gemm(a_kc, b_kc, M, N, K, A, lda, B, ldb, out, bias=None, act=0, aux_in=None, aux_out=None, residual=None,
         drop=NO_DROP, alpha=1.0, colsum_a=None, b_pre=None, accumulate=False, rowstats=None, precision=None,
         replay=False, a_amax=None, b_amax=None, c_amax=None, a_drop=NO_DROP, range_flag=None, row_skip=NO_DROP):
    """replay=True: `drop` replays a forward site's mask in backward (not a new site for ops.DropRecorder).
    b_pre = WeightPlanes.get(...) = (planes, weight amax slot) or None; a_amax / b_amax: the operands' amax slots (f16x3; a
    missing slot of A - or of B for a weight gradient - is filled by the stand-alone reduction); c_amax: slot that receives
    the bound of the values stored to `out`.  a_drop: a row-group (DropPath) mask on the rows of A - fp16 kernels only, see
    `masked_grad`.  row_skip (SampleSkip): the row groups of a DropPath site whose rows of the result are multiplied by 0 later (forward)
    or whose rows of A are zeros (backward): the fp16 kernels leave out the tiles (forward, dgrad) or K-steps (weight gradient) inside them."""
    # (this wrapper runs for a third of a step's launches: the optional arguments are tested in line instead of through _ptr / _chk,
    # ~3 us of its ~9 us of interpreter time)
    for t in (A, B, out, bias, aux_in, aux_out, residual, colsum_a):
        if t is not None and not (t.is_cuda and t.dtype is torch.float32):
            _chk(t)
    prec = GEMM_PRECISION if precision is None else precision
    planes = None
    if b_pre is not None:
        planes, b_amax = b_pre
    if prec == 6:
        kid = _gemm_kernel_id(a_kc, b_kc, M, N, K, 6, planes is not None)
        if kid == 5 or kid == 7:                # fp16 forward / dgrad kernel
            if a_amax is None:
                a_amax = amax_of(A)
            ar = eval_arithmetic.current
            if ar is not None and precision is None:
                prec = eval_launch_precision(ar.name, prec, kid, _autograd_off(), a_drop.on or row_skip.on)
                ar.switched += prec == 7
        elif kid == 6:                          # fp16 weight-gradient kernel
            if a_amax is None:
                a_amax = amax_of(A)
            if b_amax is None:
                b_amax = amax_of(B)
        else:                                   # runs as bf16x6 without planes
            planes = None
    wsb = _gemm_ws_bytes(M, N, K)
    ws, wsn = (None, 0)
    if wsb > 0:
        ws, wsn = _ws(wsb, A.device)
    seed = _S._cur.rng.seed_for(A.device, drop, a_drop, row_skip)
    if DropRecorder.sites is not None and not replay:
        DropRecorder.note(drop, "elem" if drop.mode == 0 else "group", M * N if drop.mode == 0 else drop.g2)
    # every launch is timed on the stream it runs on, also those that share the device with a kernel of another stream:
    # the population (and the average duration) is then the same as in a rocprofv3 kernel trace of the same command
    pe = None
    if GemmProbe.armed:
        kid = _gemm_kernel_id(a_kc, b_kc, M, N, K, prec, planes is not None)
        pe = GemmProbe.begin(kid)
    rc = lib().npvp_gemm_f32_skip(
        a_kc, b_kc, M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb, out.data_ptr(), out.stride(0),
        None if bias is None else bias.data_ptr(), act, None if aux_in is None else aux_in.data_ptr(),
        None if aux_out is None else aux_out.data_ptr(), None if residual is None else residual.data_ptr(),
        0 if residual is None else residual.stride(0), drop.p, drop.mode, drop.g1, drop.g2,
        None if seed is None else seed.data_ptr(), drop.salt, alpha, prec, None if colsum_a is None else colsum_a.data_ptr(),
        None if planes is None else planes.data_ptr(), 1 if accumulate else 0, None if rowstats is None else rowstats.data_ptr(),
        None if a_amax is None else a_amax.data_ptr(), None if b_amax is None else b_amax.data_ptr(),
        None if c_amax is None else c_amax.data_ptr(), None if range_flag is None else range_flag.data_ptr(),
        a_drop.p, a_drop.g1, a_drop.g2, a_drop.salt, row_skip.p, row_skip.g1, row_skip.g2, row_skip.salt,
        None if ws is None else ws.data_ptr(), wsn, _stream())
    if rc:
        check(rc, "npvp_gemm_f32_skip")
    if pe is not None:
        GemmProbe.end(pe, 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N), (a_kc, b_kc), kid)
    return out


@functools.lru_cache(maxsize=None)
def _gemm_kernel_id(a_kc, b_kc, M, N, K, prec, has_planes):
    """npvp_gemm_kernel_id, remembered per shape (a pure function of its arguments; one C call less per GEMM)"""
    return lib().npvp_gemm_kernel_id(a_kc, b_kc, M, N, K, prec, int(has_planes))


@functools.lru_cache(maxsize=None)
def _gemm_ws_bytes(M, N, K):
    return lib().npvp_gemm_workspace_bytes(M, N, K)


def _planes(w, want, R):
    return WeightPlanes.get(w, want) if R >= 256 else None


def _new_slot(dev, want=True):
    """a fresh amax slot for a tensor a kernel is about to produce, when the GEMM mode uses them"""
    return AmaxSlot.new(dev) if (want and GEMM_PRECISION == 6) else None


# --------------------------------------------------------------------------- linear backward: the plan
# Where the weight gradient of y = x w^T + b goes is decided once each: by `linear_bwd_plan` when the layer's backward runs, by
# `wgrad_plan` when the weight-gradient launch is enqueued (possibly later, inside WgradStream.flush).  Pure functions of shapes
# (R token rows: dy [R, N], x [R, K], dw [N, K]) and plain facts, remembered per argument tuple; the callers read tensors and context.
def _sunk(sk, want_b):
    """a sink exists and takes exactly the gradients wanted (it has a bias slot iff there is a bias gradient)"""
    return bool(sk) and want_b == (sk[1] is not None)


def _h16(N, K, R, precision):
    """the fp16 weight-gradient kernel takes this shape: its operands need amax slots, its launch watches the range flag"""
    return precision == 6 and _gemm_kernel_id(0, 0, N, K, R, 6, False) == 6


LinearBwdPlan = namedtuple("LinearBwdPlan", "fused reduction sunk on_grad_stream urgent fill_slots")
WgradPlan = namedtuple("WgradPlan", "route precision watch")


@functools.lru_cache(maxsize=None)
def linear_bwd_plan(R, N, K, precision, sunk, grad_stream, guard_quiet=True, unit_strides=True, planes=False, fused_on=False,
                    fused_with_stream=False, max_rows=0):
    """fused: dgrad + weight gradient in ONE launch (FusedLinearBwd), its split-K `reduction` "chained" or "queued".  Else two launches,
    the weight gradient `sunk` or returned; sunk `on_grad_stream` as a closure (`urgent`: flushed at once) or here, with `fill_slots`
    after its operands' amax slots were filled on the CURRENT stream (the gradient stream is ordered after this one: a slot first
    filled there would be read here unordered).  guard_quiet: the range guard is neither in fallback nor strict; unit_strides: of dy,
    x and the weight-gradient slice; planes: the weight has D-planes; fused_on, fused_with_stream, max_rows: FusedLinearBwd's knobs."""
    if (fused_on and precision == 6 and sunk and R <= max_rows and (fused_with_stream or not grad_stream) and guard_quiet
            and unit_strides and planes and lib().npvp_linear_bwd_f16_takes(R, N, K) and WgradChain.takes(N, K, R)):
        return LinearBwdPlan(True, "queued" if grad_stream else "chained", False, False, False, False)
    on_side = sunk and grad_stream
    return LinearBwdPlan(False, None, sunk, on_side, on_side and 2.0 * R * N * K >= 3e10, sunk and _h16(N, K, R, precision))


@functools.lru_cache(maxsize=None)
def wgrad_plan(N, K, R, precision, wgrad_precision, accumulate, masked, fallback, strict, in_flush, grad_stream, listener,
               chain_on, unit_strides):
    """route "strict" (scratch result, poll, one bf16x6 retry), "chained" (npvp_wgrad_f16_chained) or "gemm" with `precision` passed down
    (None, 4, WGRAD_PRECISION); watch: the launch raises the range flag.  accumulate: into a sink slice; masked: a row-group mask rides
    in the launch (it needs the fp16 kernel: it stays there); listener: a data-parallel one is set.  Chained: on the gradient stream
    (in_flush), or - without one (the single-stream step that is captured into a graph) - on the current stream, where the pending
    reduction rides in the next weight-gradient or fused launch and ReduceQueue.finish() runs the last one.  Not without a gradient
    stream under data parallelism: a bucket's all-reduce must not overtake a reduction that is not enqueued yet."""
    prec = wgrad_precision if precision == 4 else None
    watch = _h16(N, K, R, precision)
    if watch and fallback and not masked:
        prec, watch = 4, False
    if watch and strict and not masked:
        return WgradPlan("strict", None, True)
    if (watch and accumulate and prec is None and chain_on and WgradChain.takes(N, K, R)
            and (in_flush or (not grad_stream and not listener)) and unit_strides):
        return WgradPlan("chained", None, True)
    return WgradPlan("gemm", prec, watch)


@functools.lru_cache(maxsize=None)
def skip_roles(node, dp, wg):
    """Which launches of a node take its SampleSkip under DROP_PATH_SKIP = dp and WGRAD_ROW_SKIP = wg ("DropPath skip").  frames:
    the MlpDWBN frame kernels; forward, dgrad: its fp16 GEMM tiles; wgrad: the K-steps of an unfused fp16 weight gradient, chained or not;
    fused: the fused dgrad + weight-gradient launch, one spec for both halves.  "self_attn": the spatial sub-layer, whose dgrads take none."""
    return {"mlpdwbn": SkipRoles(dp, dp, dp, dp and wg, dp), "self_attn": SkipRoles(False, False, False, wg, wg)}[node]


def linear_fwd(x, w, b, act=0, aux_out=None, residual=None, drop=NO_DROP, rowstats=None, x_amax=None, y_amax=None):
    """y[R,N] = epilogue(x[R,K] w[N,K]^T); rowstats [R/64, N/64, 2] receives the frame-statistics partials of y;
    x_amax: x's amax slot if its producer filled one; y_amax: slot to receive the bound of y"""
    R, K = x.shape
    N = w.shape[0]
    y = torch.empty(R, N, dtype=torch.float32, device=x.device)
    return gemm(1, 1, R, N, K, x, x.stride(0), w, w.stride(0), y, bias=b, act=act, aux_out=aux_out, residual=residual,
                drop=drop, b_pre=_planes(w, "F", R), rowstats=rowstats, a_amax=x_amax, c_amax=y_amax)


def linear_frame_stats_supported(R, N):
    """the forward GEMM can emit the frame-LayerNorm statistics of its output (frames of 64 token rows)"""
    return GEMM_PRECISION in (4, 6) and R % 64 == 0 and N % 128 == 0


def linear_dgrad(dy, w, act=0, aux_in=None, drop=NO_DROP, residual=None, dy_amax=None, dx_amax=None, a_drop=NO_DROP, out=None,
                 accumulate=False, row_skip=NO_DROP):
    """dx[R,K] = epilogue((a_drop mask on the rows of dy) dy[R,N] w[N,K]); out / accumulate: into (added to) an existing [R,K] buffer"""
    R, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(R, K, dtype=torch.float32, device=dy.device) if out is None else out
    return gemm(1, 0, R, K, N, dy, dy.stride(0), w, w.stride(0), dx, act=act, aux_in=aux_in, drop=drop, residual=residual,
                b_pre=_planes(w, "D", R), replay=True, a_amax=dy_amax, c_amax=dx_amax, a_drop=a_drop, accumulate=accumulate,
                row_skip=row_skip)


def masked_grad(dy2, drop, w):
    """The gradient that flows into a linear whose output went through `drop` (dropout or DropPath): -> (dz, a_drop).  A DropPath
    (row-group) mask is handed to the dgrad and weight-gradient GEMMs as `a_drop` when both run on the fp16 kernels - they fold
    it into the scale of the rows they stage, so no masked copy of dy is written or read (2 passes over [R, C] and one launch
    per site); every other case applies the mask here (npvp_drop_apply)."""
    if not drop.on:
        return dy2, NO_DROP
    R, N = dy2.shape
    K = w.shape[1]
    if (drop.mode == 1 and drop.g1 % 16 == 0 and drop.p < 0.5 and GEMM_PRECISION == 6 and R <= DROP_PATH_IN_GEMM_ROWS
            and _planes(w, "D", R) is not None and _gemm_kernel_id(1, 0, R, K, N, 6, True) in (5, 7) and _h16(N, K, R, 6)):
        return dy2, drop
    return drop_apply(dy2, drop), NO_DROP


# Up to this many token rows.  Rounds 3 - 4 limited it to 32 768 (the launch-bound shards: c4 36.4 -> 35.1 ms; on c2 the step did
# not change then, 245.6 vs 246.2 ms, while the dgrad launches' event-pair rate fell - the masked epilogues still divided per
# element).  With the multiply-shift group index (round 4, end) the masked launch costs what the unmasked one does, and round 5's
# in-process A/B at c2 (tools/ab_bench.py: A, B, A, B on one box) reads 233.4 / 232.8 ms with the limit against 232.4 / 232.2
# without: no limit any more (20 drop_apply passes over [114 688 x 512] per step gone).
DROP_PATH_IN_GEMM_ROWS = 1 << 30


def linear_wgrad(dy, x, with_bias_grad=False, into=None, into_b=None, dy_amax=None, x_amax=None, a_drop=NO_DROP, row_skip=NO_DROP):
    """dw[N,K] = dy[R,N]^T x[R,K]; with_bias_grad also returns db[N] = column sums of dy, accumulated by the same
    kernel while it stages dy (no separate reduction pass).  into / into_b: ACCUMULATE into these existing
    gradient slices instead of allocating results (GradSink).  Range of the fp16 arithmetic: RangeGuard.  row_skip (SampleSkip): row groups
    in which dy is zero - the fp16 weight-gradient kernel leaves their K-steps out, chained or not (same bits); every other route ignores it."""
    R, N = dy.shape
    K = x.shape[1]
    acc = into is not None
    dw = into if acc else torch.empty(N, K, dtype=torch.float32, device=dy.device)
    db = (into_b if acc else torch.empty(N, dtype=torch.float32, device=dy.device)) if with_bias_grad else None
    c = _S._cur
    g = c.range_guard
    plan = wgrad_plan(N, K, R, GEMM_PRECISION, WGRAD_PRECISION, acc, a_drop.on, g.fallback, g.strict, c.wgrad.in_flush, c.wgrad.enabled,
                      c.grad_sink.listener is not None, c.chain.enabled, dy.stride(1) == 1 and x.stride(1) == 1 and dw.stride(1) == 1)
    flag = g.flag(dy.device) if plan.watch else None
    if plan.route == "strict":
        # into a scratch result first, so that a flagged launch leaves the accumulation target untouched
        tw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
        tb = torch.empty(N, dtype=torch.float32, device=dy.device) if with_bias_grad else None
        gemm(0, 0, N, K, R, dy, dy.stride(0), x, x.stride(0), tw, colsum_a=tb, a_amax=dy_amax, b_amax=x_amax, range_flag=flag)
        if g.poll(dy.device):
            g.fallback = False             # (strict mode repairs launch by launch)
            gemm(0, 0, N, K, R, dy, dy.stride(0), x, x.stride(0), tw, colsum_a=tb, precision=4)
        if acc:
            dw.add_(tw)
            if tb is not None:
                db.add_(tb)
        else:
            dw, db = tw, tb
    elif plan.route == "chained":
        c.chain.launch(dy, x, dw, db, amax_of(dy, dy_amax), amax_of(x, x_amax), a_drop, flag, row_skip)
    else:
        gemm(0, 0, N, K, R, dy, dy.stride(0), x, x.stride(0), dw, colsum_a=db, accumulate=acc, precision=plan.precision, a_amax=dy_amax,
             b_amax=x_amax, a_drop=a_drop, range_flag=flag, row_skip=row_skip)
    return (dw, db) if with_bias_grad else dw


class FusedLinearBwd:
    """dgrad + weight gradient of one linear layer as ONE launch (include/npvp_hip.h, npvp_linear_bwd_f16) - for the shapes on which
    each of the two alone leaves half the chip idle: small-tile dgrads with at least 1 024 and at most MAX_ROWS token rows (the
    8-clip shards of the data-parallel configurations; the large workloads keep the two-stream schedule).  Its split-K reduction is
    the only in-place gradient write: queued for the gradient stream, where those are serialised, or chained without one."""
    enabled = True
    MAX_ROWS = 16384
    # Beside a gradient stream the two launches on two streams are the better schedule wherever the GPU is the bound (in-process
    # A/Bs, profiles/r05_ab_knobs.txt: c4 shard eager 30.5 ms unfused / 31.3 fused, c2 233.3 / 234.3, c1 with 20 480-row layers
    # fused 89.8 against 86.2): the fused launch is for the step WITHOUT a gradient stream - the single-stream capture that is
    # replayed from a graph.  with_gradient_stream = True takes it in the eager two-stream step too: fewer launches (934 instead of
    # 1 160 per c4 step), which is what a host-bound step wants (bench.py tries both under data parallelism, where the step
    # cannot be replayed from a graph).
    with_gradient_stream = False

    @classmethod
    def takes(cls, R, N, K):
        """the shape, with everything else in favour (linear_bwd_plan)"""
        return linear_bwd_plan(R, N, K, 6, True, False, True, True, True, True, False, cls.MAX_ROWS).fused


def linear_bwd(dy, x, w, b, sk, act=0, aux_in=None, drop=NO_DROP, residual=None, dy_amax=None, dx_amax=None, a_drop=NO_DROP, skip=NO_SKIP):
    """The backward of y = x w^T + b given dy [R, N]: -> dx = epilogue((a_drop mask) dy w), gw, gb - the weight (+ bias) gradient goes
    into the sink `sk` (-> None, None) or is returned.  One launch where FusedLinearBwd takes the shape, else the dgrad on this
    stream and the weight gradient on the gradient stream as before.  skip (SampleSkip): samples in whose rows dy is zero - where its roles say
    so, the dgrad leaves their tiles out, the fp16 weight gradient their K-steps (x is not read there), the fused launch both with ONE spec."""
    R, N = dy.shape
    K = w.shape[1]
    has_b = b is not None
    c = _S._cur
    sunk = _sunk(sk, has_b)
    pl = _planes(w, "D", R)
    plan = linear_bwd_plan(R, N, K, GEMM_PRECISION, sunk, c.wgrad.enabled, not (c.range_guard.fallback or c.range_guard.strict),
                           dy.stride(1) == 1 and x.stride(1) == 1 and (not sunk or sk[0][0].stride(1) == 1), pl is not None,
                           FusedLinearBwd.enabled, FusedLinearBwd.with_gradient_stream, FusedLinearBwd.MAX_ROWS)
    if not plan.fused:
        dx = linear_dgrad(dy, w, act=act, aux_in=aux_in, drop=drop, residual=residual, dy_amax=dy_amax, dx_amax=dx_amax, a_drop=a_drop,
                          row_skip=skip.dgrad)
        return (dx, *_lin_grads(dy, x, w, b, sk, a_drop=a_drop, plan=plan, row_skip=skip.wgrad))
    planes, w_amax = pl
    gw, gb = sk[0][0], (sk[1][0] if has_b else None)
    dev = dy.device
    dy_amax, x_amax = amax_of(dy, dy_amax), amax_of(x)
    dx = torch.empty(R, K, dtype=torch.float32, device=dev)
    ws, wsn = _ws(c.chain.workspace_bytes(N, K, R), dev)
    st = _stream()
    rs = skip.fused
    outs = (gw.data_ptr(),) if gb is None else (gw.data_ptr(), gb.data_ptr())
    later = c.chain if plan.reduction == "chained" else c.reduce       # who runs this launch's split-K reduction
    job_addr, prev_addr = later.job_slot(st, outs)
    pe = GemmProbe.begin(8)
    check(lib().npvp_linear_bwd_f16_skip(
        R, N, K, dy.data_ptr(), dy.stride(0), dy_amax.data_ptr(), planes.data_ptr(), w_amax.data_ptr(), dx.data_ptr(), dx.stride(0),
        act, _ptr(aux_in), _ptr(residual), 0 if residual is None else residual.stride(0), drop.p, drop.mode, drop.g1, drop.g2,
        drop.salt, _ptr(dx_amax), x.data_ptr(), x.stride(0), x_amax.data_ptr(), gw.data_ptr(), gw.stride(0), _ptr(gb),
        _ptr(c.range_guard.flag(dev)), a_drop.p, a_drop.g1, a_drop.g2, a_drop.salt, rs.p, rs.g1, rs.g2, rs.salt,
        _ptr(c.rng.seed_for(dev, drop, a_drop, rs)), prev_addr, job_addr, ws.data_ptr(), wsn, st), "npvp_linear_bwd_f16_skip")
    GemmProbe.end(pe, 4.0 * R * N * K, 4.0 * (2 * R * N + 2 * R * K + 2 * N * K), (1, 0), 8)
    later.job_added(st, outs, (ws, gw, gb), sk)
    return dx, None, None


def colsum(x):
    R, N = x.shape
    L = lib()
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws, wsn = _ws(L.npvp_colsum_workspace_bytes(R, N), x.device)
    check(L.npvp_colsum(_ptr(x), R, N, x.stride(0), _ptr(out), 0, _ptr(ws), wsn, _stream()), "npvp_colsum")
    return out


def drop_apply(x2d, drop):
    out = torch.empty_like(x2d)
    slot = _new_slot(x2d.device)
    check(lib().npvp_drop_apply(_ptr(x2d), _ptr(out), x2d.shape[0], x2d.shape[1], drop.p, drop.mode, drop.g1, drop.g2,
                                _ptr(_S._cur.rng.seed_tensor(x2d.device)), drop.salt, _ptr(slot), _stream()), "npvp_drop_apply")
    return tag_amax(out, slot)


def transpose(x):
    """[B,R,C] -> [B,C,R]"""
    _chk(x)
    x = _c(x)
    B, R, C = x.shape
    out = torch.empty(B, C, R, dtype=torch.float32, device=x.device)
    check(lib().npvp_transpose(_ptr(x), _ptr(out), B, R, C, _stream()), "npvp_transpose")
    return out


def reduce_mid(x, scale=1.0, out=None, accumulate=False):
    """[A,B,C] -> [A,C]: scale * sum over B (into `out`, added to it with accumulate)"""
    _chk(x)
    x = _c(x)
    A, B, C = x.shape
    if out is None:
        out = torch.empty(A, C, dtype=torch.float32, device=x.device)
    check(lib().npvp_reduce_mid(_ptr(x), _ptr(out), A, B, C, scale, 1 if accumulate else 0, _stream()), "npvp_reduce_mid")
    return out


class ActSink:
    """The gradient of an activation that feeds MANY sub-layers - a positional table (~30 per step), the event latent (16), the
    decoder's memory and its fused key (8 each) - summed IN PLACE by its consumers' backward kernels (the `accumulate` flag of
    npvp_posfuse_bwd / npvp_reduce_mid / the dgrad GEMM) instead of by one autograd add kernel per consumer (75 launches per
    step).  `fan_out(t)` returns t as seen through an identity node that owns a sink; a consumer that finds `t._npvp_sink` writes
    its share into `sink.target(...)` and returns None for that input; the identity node's backward hands the buffer on (plus
    whatever consumers without the in-place route returned the usual way)."""
    __slots__ = ("buf",)
    enabled = True

    def __init__(self):
        self.buf = None

    def target(self, shape, dev):
        """-> (buffer, accumulate): the first contribution of a backward pass writes, the others add"""
        if self.buf is None:
            self.buf = torch.empty(shape, dtype=torch.float32, device=dev)
            return self.buf, False
        if self.buf.numel() != torch.Size(shape).numel():
            raise RuntimeError(f"ActSink: a consumer contributes a gradient of shape {tuple(shape)} to a buffer of shape {tuple(self.buf.shape)}")
        return self.buf, True

    @staticmethod
    def of(t):
        return None if t is None else getattr(t, "_npvp_sink", None)


class _FanOut(_Function):
    @staticmethod
    def forward(ctx, t, sink):
        ctx.sink = sink
        ctx.set_materialize_grads(False)
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        buf, ctx.sink.buf = ctx.sink.buf, None
        if buf is None:
            return g, None
        if g is not None:
            buf.add_(g.reshape(buf.shape))
        return buf, None


def fan_out(t):
    """t for consumers that can sum their gradient contributions in place (ActSink); anything else sees a plain tensor"""
    if t is None or not (ActSink.enabled and t.is_cuda and t.requires_grad and torch.is_grad_enabled()):
        return t
    sink = ActSink()
    out = _FanOut.apply(t, sink)
    out._npvp_sink = sink
    return out


def broadcast_mid(x, B, scale=1.0):
    """[A,C] -> [A,B,C]"""
    _chk(x)
    x = _c(x)
    A, C = x.shape
    out = torch.empty(A, B, C, dtype=torch.float32, device=x.device)
    check(lib().npvp_broadcast_mid(_ptr(x), _ptr(out), A, B, C, scale, _stream()), "npvp_broadcast_mid")
    return out


# --------------------------------------------------------------------------- autograd Functions
class _Transpose(_Function):
    @staticmethod
    def forward(ctx, x):
        remember(ctx)
        return transpose(x)

    @scoped
    def backward(ctx, g):
        return transpose(g)


class _MeanMid(_Function):
    """[A,B,C] -> [A,C] mean over B (event coding = mean over T, ref/models/Predictor.py:346)"""

    @staticmethod
    def forward(ctx, x):
        remember(ctx)
        ctx.B = x.shape[1]
        return reduce_mid(x, 1.0 / x.shape[1])

    @scoped
    def backward(ctx, g):
        return broadcast_mid(g, ctx.B, 1.0 / ctx.B)


class _L1Mean(_Function):
    """lam * mean|a - b| (ref/models/criterion.py:99-121 with norm_dim None); the gradient goes to `a` only - the second operand of
    the Stage-2 losses is the ground truth.  One fused pass forward, one backward, and no torch reduction: a captured step must not
    contain memset nodes (npvp_hip.h npvp_l1_mean)."""

    @staticmethod
    def forward(ctx, a, b, lam):
        remember(ctx)
        _chk(a, b)
        if a.shape != b.shape:
            raise RuntimeError(f"l1_mean: shapes differ: {tuple(a.shape)} / {tuple(b.shape)}")
        a, b = _c(a), _c(b)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws, wsn = _ws(4096, a.device)
        check(lib().npvp_l1_mean(_ptr(a), _ptr(b), a.numel(), float(lam), _ptr(out), _ptr(ws), wsn, _stream()), "npvp_l1_mean")
        ctx.save_for_backward(a, b)
        ctx.lam = float(lam)
        return out

    @scoped
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        _chk(g)
        da = torch.empty_like(a)
        check(lib().npvp_l1_mean_bwd(_ptr(a), _ptr(b), a.numel(), _ptr(_c(g)), ctx.lam, _ptr(da), _stream()), "npvp_l1_mean_bwd")
        return da, None, None


def l1_mean(a, b, lam=1.0):
    if b.requires_grad:
        raise RuntimeError("l1_mean: only the first operand takes a gradient (the Stage-2 losses compare against ground truth)")
    return _L1Mean.apply(a, b, lam)


class _SumAll(_Function):
    """sum of every element -> device scalar, in a fixed order (npvp_hip.h npvp_sum_all)"""

    @staticmethod
    def forward(ctx, x):
        _chk(x)
        ctx.shape = x.shape
        x = _c(x)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ws, wsn = _ws(4096, x.device)
        check(lib().npvp_sum_all(_ptr(x), x.numel(), _ptr(out), _ptr(ws), wsn, _stream()), "npvp_sum_all")
        return out

    @staticmethod
    def backward(ctx, g):
        return g.expand(ctx.shape)


def sum_all(x):
    return _SumAll.apply(x)


class _LayerNorm(_Function):
    @staticmethod
    def forward(ctx, x, w, b, eps, relu):
        remember(ctx)
        _chk(x, w, b)
        x2 = _c(x).reshape(-1, x.shape[-1])
        y, st = _raw_ln_fwd(x2, w, b, eps, int(relu))
        ctx.save_for_backward(x2, w, b, st)
        ctx.relu, ctx.shape = int(relu), x.shape
        ctx.sink = _ln_sink(w, b)
        return y.reshape(x.shape)

    @scoped
    def backward(ctx, dy):
        x2, w, b, st = ctx.saved_tensors
        dx, dw, db = _raw_ln_bwd(_c(dy).reshape(x2.shape), x2, w, b, st, None, ctx.sink, ctx.relu)
        return dx.reshape(ctx.shape), dw, db, None, None


def _ln_sink(w, b):
    sw, sb = _S._cur.grad_sink.slot(w), _S._cur.grad_sink.slot(b)
    return (sw, sb) if (sw is not None and sb is not None) else None


def _sink_mode(sk):
    """`accumulate` argument of the norm backward entry points: 0 plain outputs, 1 accumulate into the gradient slots
    on this stream, 2 leave the partial sums in the workspace - their reduction into the slots then runs on the
    gradient stream (WgradStream), where EVERY in-place gradient write is serialised."""
    return 0 if not sk else (2 if (_S._cur.wgrad.enabled or _S._cur.reduce.enabled) else 1)


def _reduce_partials(sk, ws, gw, gb, direct, job, what, tail, accumulated):
    """The parameter-gradient partials a backward kernel left in `ws` -> the gradient slices gw / gb of the sink `sk`: as a job of
    the ReduceQueue (`job`, the library's *_job form), else by `direct` on the gradient stream, else - neither of the two - on
    this stream: nothing is left to do when `accumulated` (the kernel added to the slices itself: _sink_mode gave 1), `direct`
    runs here otherwise.  tail: the scalar arguments both forms take after the three addresses."""
    if _S._cur.reduce.enabled:
        _S._cur.reduce.add(job, what + " (ReduceQueue job)", (_ptr(ws), _ptr(gw), _ptr(gb)) + tail, (gw.data_ptr(), gb.data_ptr()), ws, sk)
        return
    # (deferred on the gradient stream: every value is bound NOW, the closure runs a few launches later)
    fn = lambda ws=ws, gw=gw, gb=gb: check(direct(_ptr(ws), _ptr(gw), _ptr(gb), *tail, _stream()), what)
    if _S._cur.wgrad.enabled:
        _S._cur.wgrad.run(fn, ws, wrote=sk)
    else:
        if not accumulated:
            fn()
        _S._cur.grad_sink.wrote(*sk)


def layernorm(x, w, b, eps=1e-5, relu=False):
    return _LayerNorm.apply(x, w, b, eps, relu)


class _LayerNormNchw(_Function):
    """LayerNorm(C) (+ReLU) over the token rows of canonical x [F, 64, C], result in the reference's (N,T,C,H,W) layout
    (ref VidHRFormer.py:150-159): one forward kernel instead of LayerNorm + transpose."""

    @staticmethod
    def forward(ctx, x, w, b, eps, relu, N, T, H, W):
        remember(ctx)
        _chk(x, w, b)
        C = x.shape[-1]
        x3 = _c(x).reshape(N * T, H * W, C)
        out = torch.empty(N, T, C, H, W, dtype=torch.float32, device=x.device)
        st = torch.empty(2, N * T * H * W, dtype=torch.float32, device=x.device)
        check(lib().npvp_layernorm_nchw_fwd(_ptr(x3), _ptr(w), _ptr(b), _ptr(out), _row(st, 0), _row(st, 1), N * T, H * W, C, eps,
                                            int(relu), _stream()), "npvp_layernorm_nchw_fwd")
        ctx.save_for_backward(x3, w, b, st)
        ctx.relu, ctx.shape = int(relu), x.shape
        ctx.sink = _ln_sink(w, b)
        return out

    @scoped
    def backward(ctx, dy):
        # dy (N,T,C,H,W) -> canonical rows (the LDS-tiled transpose), then the row-wise LayerNorm backward: a fused backward
        # through the forward kernel's tile was 3x slower than these two kernels
        x3, w, b, st = ctx.saved_tensors
        F_, P, C = x3.shape
        dy = _c(dy)
        dy2 = torch.empty(F_ * P, C, dtype=torch.float32, device=dy.device)
        check(lib().npvp_transpose(_ptr(dy), _ptr(dy2), F_, C, P, _stream()), "npvp_transpose")
        dx, dw, db = _raw_ln_bwd(dy2, x3.reshape(F_ * P, C), w, b, st, None, ctx.sink, ctx.relu)
        return (dx.reshape(ctx.shape), dw, db) + (None,) * 6


def layernorm_nchw_supported(x, H, W):
    return x.is_cuda and H * W == 64 and x.shape[-1] in (256, 512)


def layernorm_nchw(x, w, b, eps, relu, N, T, H, W):
    """canonical (N,T,H,W,C) -> LayerNorm (+ReLU) -> (N,T,C,H,W)"""
    return _LayerNormNchw.apply(x, w, b, eps, relu, N, T, H, W)


class _LayerNormRes(_Function):
    """(x, LN(x)) for the pre-norm residual pattern  x + f(LN(x))  of every sub-layer (ref VidHRFormer.py:87-112).
    Returning x through the Function lets backward fold the residual branch's gradient into the LayerNorm backward
    kernel (dx = d_residual + LN'(dy)) instead of leaving a separate [R, C] add to autograd."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        remember(ctx)
        _chk(x, w, b)
        x2 = _c(x).reshape(-1, x.shape[-1])
        y, st = _raw_ln_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, w, b, st)
        ctx.shape = x.shape
        ctx.sink = _ln_sink(w, b)
        return x.view_as(x), y.reshape(x.shape)

    @scoped
    def backward(ctx, dres, dy):
        if dy is None:
            return dres, None, None, None
        x2, w, b, st = ctx.saved_tensors
        dr2 = None if dres is None else _c(dres).reshape(x2.shape)
        dx, dw, db = _raw_ln_bwd(_c(dy).reshape(x2.shape), x2, w, b, st, dr2, ctx.sink)
        return dx.reshape(ctx.shape), dw, db, None


def layernorm_res(x, w, b, eps=1e-5):
    """returns (x, LN(x)); use the returned x as the residual operand"""
    return _LayerNormRes.apply(x, w, b, eps)


class _PosFuse(_Function):
    """y = GroupNorm1(x + add) * (1 + gamma) + beta on [N*T, PF] frames (ref submodules.py:432-454)."""

    @staticmethod
    def forward(ctx, x, add, beta, gamma, N, T):
        remember(ctx)
        _chk(x, add, beta, gamma)
        x = _c(x)
        beta = _c(beta)
        add_c = None if add is None else _c(add)
        gamma_c = None if gamma is None else _c(gamma)
        y, st = _raw_posfuse_fwd(x, add_c, beta, gamma_c, N, T)
        ctx.save_for_backward(x, add_c, gamma_c, st)
        ctx.N, ctx.T, ctx.PF = N, T, x.numel() // (N * T)
        ctx.beta_shape = beta.shape
        return y

    @scoped
    def backward(ctx, dy):
        x, add, gamma, st = ctx.saved_tensors
        N, T, PF = ctx.N, ctx.T, ctx.PF
        dy = _c(dy)
        du, dbeta, dgamma = _posfuse_bwd_call(dy, x, add, gamma, st, N, T, PF, ctx.beta_shape, ctx.needs_input_grad[2],
                                              gamma is not None and ctx.needs_input_grad[3])
        dadd = reduce_mid(du.view(N, T, PF)).view(add.shape) if (add is not None and ctx.needs_input_grad[1]) else None
        return du, dadd, dbeta, dgamma, None, None


def _posfuse_bwd_call(dy, x, add, gamma, st, N, T, PF, beta_shape, want_beta, want_gamma, beta_sink=None, gamma_sink=None):
    """-> du, dbeta, dgamma: one entry point; the sums over the batch come out of the apply pass when the shape allows
    (npvp_posfuse_bwd_fused), else through a dy*uhat scratch and two reductions inside the library.  With sinks (ActSink) the
    table gradients are accumulated in place and None is returned for them."""
    L = lib()
    du = torch.empty_like(x)
    acc = False
    sunk = beta_sink is not None and want_beta and (not want_gamma or gamma_sink is not None)
    if sunk:
        # (one accumulate flag for both tables: they are sunk together - a fresh pair is written, an existing pair added to)
        dbeta, acc = beta_sink.target(beta_shape, x.device)
        dgamma = None
        if want_gamma:
            dgamma, acc_g = gamma_sink.target(gamma.shape, x.device)
            if acc_g != acc:
                # the kernel takes ONE accumulate flag: a pair out of step (one table sunk alone by some consumer) would have its
                # second table accumulated into uninitialised memory - bring the fresh buffer to zero and accumulate into both
                (dgamma if not acc_g else dbeta).zero_()
                acc = True
    else:
        dbeta = torch.empty(beta_shape, dtype=torch.float32, device=x.device) if want_beta else None
        dgamma = torch.empty(gamma.shape, dtype=torch.float32, device=x.device) if want_gamma else None
    dyxh = torch.empty_like(x) if (want_gamma and not L.npvp_posfuse_bwd_fused(N, T, PF)) else None
    ws, wsn = _ws(8 * N * T, x.device)
    check(L.npvp_posfuse_bwd(_ptr(dy), _ptr(x), _ptr(add), _ptr(gamma), _row(st, 0), _row(st, 1), _ptr(du), _ptr(dyxh), _ptr(dbeta),
                             _ptr(dgamma), N, T, PF, 1 if acc else 0, _ptr(ws), wsn, _stream()), "npvp_posfuse_bwd")
    return (du, None, None) if sunk else (du, dbeta, dgamma)


def posfuse(x, add, beta, gamma, N, T):
    return _PosFuse.apply(x, add, beta, gamma, N, T)


class _PosFuseInstance(_Function):
    """PosFeatFuser with param_free_norm_type='instance' (ref submodules.py:427-431): statistics per (frame, channel) over the
    H*W pixels.  x (N,T,H,W,C) channels-last; beta / gamma [T*H*W, C]; add (N,H,W,C) or None."""

    @staticmethod
    def forward(ctx, x, add, beta, gamma, N, T):
        remember(ctx)
        _chk(x, add, beta, gamma)
        x = _c(x)
        C = x.shape[-1]
        P = x.numel() // (N * T * C)
        beta = _c(beta)
        add_c = None if add is None else _c(add)
        gamma_c = None if gamma is None else _c(gamma)
        y = torch.empty_like(x)
        st = torch.empty(2, N * T, C, dtype=torch.float32, device=x.device)
        slot = _new_slot(x.device)
        check(lib().npvp_posfuse_instance_fwd(_ptr(x), _ptr(add_c), _ptr(beta), _ptr(gamma_c), _ptr(y), _row(st, 0), _row(st, 1), N, T, P,
                                              C, 1e-5, _ptr(slot), _stream()), "npvp_posfuse_instance_fwd")
        tag_amax(y, slot)
        ctx.save_for_backward(x, add_c, gamma_c, st)
        ctx.cfg = (N, T, P, C, beta.shape)
        return y

    @scoped
    def backward(ctx, dy):
        x, add, gamma, st = ctx.saved_tensors
        N, T, P, C, beta_shape = ctx.cfg
        dy = _c(dy)
        du = torch.empty_like(x)
        dyxh = torch.empty_like(x) if (gamma is not None and ctx.needs_input_grad[3]) else None
        check(lib().npvp_posfuse_instance_bwd(_ptr(dy), _ptr(x), _ptr(add), _ptr(gamma), _row(st, 0), _row(st, 1), _ptr(du), _ptr(dyxh),
                                              N, T, P, C, _stream()), "npvp_posfuse_instance_bwd")
        PF = P * C
        dadd = reduce_mid(du.view(N, T, PF)).view(add.shape) if (add is not None and ctx.needs_input_grad[1]) else None
        dbeta = reduce_mid(dy.view(1, N, T * PF)).view(beta_shape) if ctx.needs_input_grad[2] else None
        dgamma = reduce_mid(dyxh.view(1, N, T * PF)).view(gamma.shape) if dyxh is not None else None
        return du, dadd, dbeta, dgamma, None, None


def posfuse_instance(x, add, beta, gamma, N, T):
    return _PosFuseInstance.apply(x, add, beta, gamma, N, T)


class _Linear(_Function):
    """y = residual + drop(x w^T + b): nn.Linear / 1x1 conv / MHA projections with the residual add
    and the dropout / drop-path that follows them in the reference fused into the GEMM epilogue."""

    @staticmethod
    def forward(ctx, x, w, b, residual, drop, frame_stats=False):
        remember(ctx)
        _chk(x, w, b, residual)
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        if x2.stride(1) != 1 or x2.stride(0) % 4 != 0:
            x2 = x2.contiguous()
        w = w if (w.stride(1) == 1 and w.stride(0) % 4 == 0) else w.contiguous()
        r2 = None if residual is None else _c(residual).reshape(-1, w.shape[0])
        ctx.save_for_backward(x2, w)
        ctx.drop, ctx.has_b, ctx.has_r, ctx.xshape = drop, b is not None, residual is not None, x.shape
        ctx.sink = _wb_sink(w, b)
        if frame_stats:
            # the GEMM's epilogue leaves per-(frame, 64-column block) partial statistics of y; a tiny kernel merges them
            R, N = x2.shape[0], w.shape[0]
            frames = R // 64
            part = torch.empty(frames * (N // 64) * 2, dtype=torch.float32, device=x.device)
            y = linear_fwd(x2, w, b, rowstats=part)
            mean = torch.empty(frames, dtype=torch.float32, device=x.device)
            rstd = torch.empty_like(mean)
            check(lib().npvp_frame_stats_finalize(_ptr(part), N // 64, 4096.0, _ptr(mean), _ptr(rstd), frames, 1e-5, _stream()),
                  "npvp_frame_stats_finalize")
            ctx.mark_non_differentiable(mean, rstd)
            ctx.set_materialize_grads(False)        # no zero-filled gradient tensors for the two statistics outputs
            return y.reshape(*x.shape[:-1], N), mean, rstd
        y = linear_fwd(x2, w, b, residual=r2, drop=drop)
        return y.reshape(*x.shape[:-1], w.shape[0])

    @scoped
    def backward(ctx, dy, *_stats_grads):
        x2, w = ctx.saved_tensors
        N = w.shape[0]
        dy2 = _c(dy).reshape(-1, N)
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            dz, ad = masked_grad(dy2, ctx.drop, w)          # (a DropPath mask rides in the two GEMMs when they can take it)
        else:
            dz, ad = (drop_apply(dy2, ctx.drop) if ctx.drop.on else dy2), NO_DROP
        dx = linear_dgrad(dz, w, a_drop=ad).reshape(ctx.xshape) if ctx.needs_input_grad[0] else None
        dw = db = None
        want_b = ctx.has_b and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw, db = _lin_grads(dz, x2, w, True if want_b else None, ctx.sink, a_drop=ad)
        elif want_b:
            db = colsum(dz)
        dres = dy if ctx.has_r else None
        return dx, dw, db, dres, None, None


def _lin_grads(dy, x, w, b, sk, a_drop=NO_DROP, plan=None, row_skip=NO_DROP):
    """weight (+ bias) gradient of y = x w^T + b (`b` only says whether there is a bias gradient to take): accumulated into the
    sink `sk` (-> None, None) - on the gradient stream when there is one - or returned.  row_skip: see linear_wgrad"""
    has_b = b is not None
    if plan is None:
        plan = linear_bwd_plan(dy.shape[0], dy.shape[1], x.shape[1], GEMM_PRECISION, _sunk(sk, has_b), _S._cur.wgrad.enabled)
    if not plan.sunk:
        g = linear_wgrad(dy, x, has_b, a_drop=a_drop, row_skip=row_skip)
        return (g[0], g[1]) if has_b else (g, None)
    a1, a2 = (amax_of(dy), amax_of(x)) if plan.fill_slots else (None, None)
    fn = lambda dy=dy, x=x, gw=sk[0][0], gb=(sk[1][0] if has_b else None), a1=a1, a2=a2, ad=a_drop, rs=row_skip: \
        linear_wgrad(dy, x, has_b, into=gw, into_b=gb, dy_amax=a1, x_amax=a2, a_drop=ad, row_skip=rs)
    if plan.on_grad_stream:
        _S._cur.wgrad.run(fn, dy, x, wrote=sk, urgent=plan.urgent)
    else:
        fn()
        _S._cur.grad_sink.wrote(*sk)
    return None, None


def _wb_sink(w, b):
    """(weight slot, bias slot or None) when BOTH gradients can be accumulated in place, else None"""
    sw = _S._cur.grad_sink.slot(w)
    if sw is None:
        return None
    if b is None or not b.requires_grad:
        return (sw, None)
    sb = _S._cur.grad_sink.slot(b)
    return (sw, sb) if sb is not None else None


def linear(x, w, b=None, residual=None, drop=NO_DROP, frame_stats=False):
    """frame_stats=True (plain bias-only linear whose rows come in frames of 64): returns (y, mean, rstd), the statistics
    a following frame LayerNorm needs, computed in the GEMM's epilogue"""
    if frame_stats:
        assert residual is None and not drop.on
    return _Linear.apply(x, w, b, residual, drop, bool(frame_stats))


class _FFN(_Function):
    """out = x + drop3(linear2(drop2(GELU(linear1(xn)))))  (ref/models/VidHRFormer.py:110-112,224-226):
    two GEMMs; bias+GELU+dropout and bias+dropout+residual live in their epilogues, and in backward the
    GELU'/dropout product is the epilogue of the dgrad GEMM."""

    @staticmethod
    def forward(ctx, xn, x, w1, b1, w2, b2, p):
        remember(ctx)
        _chk(xn, x, w1, b1, w2, b2)
        C = xn.shape[-1]
        xn2, x2 = _c(xn).reshape(-1, C), _c(x).reshape(-1, C)
        h, a, y, d2, d3 = _ffn_fwd(xn2, x2, w1, b1, w2, b2, p)
        ctx.save_for_backward(xn2, h, a, w1, w2)
        ctx.d2, ctx.d3, ctx.shape = d2, d3, x.shape
        s1, s2 = _wb_sink(w1, b1), _wb_sink(w2, b2)
        ctx.sink = (s1, s2) if (_sunk(s1, True) and _sunk(s2, True)) else None
        return y.reshape(x.shape)

    @scoped
    def backward(ctx, dy):
        xn2, h, a, w1, w2 = ctx.saved_tensors
        C = xn2.shape[1]
        dy2 = _c(dy).reshape(-1, C)
        dz2, ad = masked_grad(dy2, ctx.d3, w2)
        sk = ctx.sink
        if sk:
            dh = linear_dgrad(dz2, w2, act=3, aux_in=h, drop=ctx.d2, a_drop=ad)
            _lin_grads(dz2, a, w2, True, sk[1], a_drop=ad)
            dxn = linear_dgrad(dh, w1)
            _lin_grads(dh, xn2, w1, True, sk[0])
            return dxn.reshape(ctx.shape), dy, None, None, None, None, None
        dw2, db2 = linear_wgrad(dz2, a, True, a_drop=ad)
        dh = linear_dgrad(dz2, w2, act=3, aux_in=h, drop=ctx.d2, a_drop=ad)
        dw1, db1 = linear_wgrad(dh, xn2, True)
        dxn = linear_dgrad(dh, w1)
        return dxn.reshape(ctx.shape), dy, dw1, db1, dw2, db2, None


def _ffn_fwd(xn2, x2, w1, b1, w2, b2, p):
    """-> h = linear1(xn2) (saved for GELU'), a = drop2(GELU(h)), y = x2 + drop3(linear2(a)), and the two dropout sites"""
    d2, d3 = Drop(p), Drop(p)
    h = torch.empty(xn2.shape[0], w1.shape[0], dtype=torch.float32, device=xn2.device)
    a_slot = _new_slot(xn2.device)
    a = tag_amax(linear_fwd(xn2, w1, b1, act=1, aux_out=h, drop=d2, y_amax=a_slot), a_slot)
    return h, a, linear_fwd(a, w2, b2, residual=x2, drop=d3), d2, d3


def ffn(xn, x, w1, b1, w2, b2, p):
    return _FFN.apply(xn, x, w1, b1, w2, b2, p)


def window_pad_geometry(H, W, ws):
    """(Hp, Wp, top, left) of ref/models/VidHRFormer.py:488-511 (PadBlock): the grid is centre-padded to the next multiple of the
    window; an odd pad puts the smaller half first.  THE place these formulas are written in npvp_amd."""
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    return Hp, Wp, (Hp - H) // 2, (Wp - W) // 2


class AttnCfg:
    """What the attention entry points take.  grid = None: the window tiles the grid (every call written before the centre-pad
    route means this).  grid = (H, W, top, left): a spatial-window site whose H x W grid the window does not tile - P and W
    describe the PADDED Hp x Wp grid the kernels run on (Hp = P / W, Wp = W), the real grid lies at (top, left) in it."""
    __slots__ = ("mode", "dim0", "P", "W", "ws", "Tq", "Tk", "heads", "mask_mode", "drop", "grid")

    def __init__(self, mode, dim0, P, W, ws, Tq, Tk, heads, mask_mode, p_drop, grid=None):
        self.mode, self.dim0, self.P, self.W, self.ws, self.Tq, self.Tk = mode, dim0, P, W, ws, Tq, Tk
        self.heads, self.mask_mode = heads, mask_mode
        self.drop = Drop(p_drop)
        self.grid = grid

    @property
    def tiles(self):
        return self.grid is None

    @classmethod
    def spatial(cls, frames, H, W, ws, heads, p_drop):
        """the spatial-window configuration of an H x W grid: the tiling one, or the centre-padded one"""
        Hp, Wp, top, left = window_pad_geometry(H, W, ws)
        grid = None if (Hp, Wp) == (H, W) else (H, W, top, left)
        return cls(0, frames, Hp * Wp, Wp, ws, 0, 0, heads, 0, p_drop, grid)

    def pad_args(self):
        """(F, H, W, Hp, Wp, top, left) as npvp_grid_center_pad / _cut take them"""
        H, W, top, left = self.grid
        return self.dim0, H, W, self.P // self.W, self.W, top, left

    @property
    def padded_rows(self):
        """rows of the padded buffers: dim0 * Hp * Wp rounded up to the 32 the weight-gradient GEMM wants (the trailing rows are zeros)"""
        return -(-self.dim0 * self.P // 32) * 32


# Sequences of at least this many rows on either side take the streaming kernels (npvp_attn_long_*: any length); shorter ones the
# kernels of npvp_attn_fwd / npvp_attn_bwd (up to 32: MFMA, 33 .. 128: generic), which end at 128.  A module constant so that
# tools/attn_bench.py and a test can lower it and compare the two routes on the same shapes.
ATTN_LONG_MIN = 129


def _attn_len(cfg):
    """(L, S): query and key rows per (group, head)"""
    return (cfg.ws * cfg.ws, cfg.ws * cfg.ws) if cfg.mode == 0 else (cfg.Tq, cfg.Tk)


def _attn_groups(cfg):
    """attention groups: (frame, window) pairs or (sample, pixel) pairs (attn_setup of csrc/attn.hip)"""
    return cfg.dim0 * (cfg.P // (cfg.ws * cfg.ws)) if cfg.mode == 0 else cfg.dim0 * cfg.P


def _attn_long(cfg):
    return max(_attn_len(cfg)) >= ATTN_LONG_MIN


def _attn_fwd_entry(cfg):
    """(function, its name) of the forward entry point that takes cfg's sequence lengths"""
    return (lib().npvp_attn_long_fwd, "npvp_attn_long_fwd") if _attn_long(cfg) else (lib().npvp_attn_fwd, "npvp_attn_fwd")


def _attn_fwd(q, k, v, o, cfg):
    hd = o.shape[1] // cfg.heads
    seed = _S._cur.rng.seed_for(q.device, cfg.drop)
    if DropRecorder.sites is not None and cfg.drop.on:      # weights tensor [groups, heads, L, S]
        L_, S_ = _attn_len(cfg)
        DropRecorder.note(cfg.drop, "elem", _attn_groups(cfg) * cfg.heads * L_ * S_)
    slot = _new_slot(q.device)
    fn, what = _attn_fwd_entry(cfg)
    check(fn(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0),
             cfg.mode, cfg.dim0, cfg.P, cfg.W, cfg.ws, cfg.Tq, cfg.Tk, cfg.heads, hd, cfg.mask_mode,
             cfg.drop.p, _ptr(seed), cfg.drop.salt, _ptr(slot), _stream()), what)
    tag_amax(o, slot)


ATTN_SAMPLES_MAX = 32      # longest sequence npvp_attn_samples_fwd takes (the one- and two-block MFMA form)


def _attn_samples_fwd(q, k, v, o, cfg, S, sample_chunk=0):
    """The sampler's encoder-decoder core (forward only, no mask, no dropout): q / o hold S * cfg.dim0 clips, sample-major, k / v the
    cfg.dim0 clips of the memory - never replicated.  Up to 32 rows per side: ONE launch of npvp_attn_samples_fwd (a wave loads a
    group's K / V tiles once for several samples).  Longer: one call of the existing forward entry points per sample slab (the slab
    of a sample is contiguous: a pointer offset), `_attn_long` choosing between them as in `_attn_fwd`, every call on the same k / v
    and the same amax slot (a slot is a maximum: exact)."""
    if cfg.mode != 1 or cfg.mask_mode != 0 or cfg.drop.on:
        raise ValueError("_attn_samples_fwd: temporal geometry without mask and dropout only")
    hd = o.shape[1] // cfg.heads
    slot = _new_slot(q.device)
    if max(cfg.Tq, cfg.Tk) <= ATTN_SAMPLES_MAX:
        check(lib().npvp_attn_samples_fwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(o), o.stride(0),
                                          S, cfg.dim0, cfg.P, cfg.Tq, cfg.Tk, cfg.heads, hd, sample_chunk, _ptr(slot), _stream()),
              "npvp_attn_samples_fwd")
    else:
        fn, what = _attn_fwd_entry(cfg)
        rows = cfg.dim0 * cfg.Tq * cfg.P          # query rows of one sample
        for s in range(S):
            check(fn(q.data_ptr() + 4 * s * rows * q.stride(0), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0),
                     o.data_ptr() + 4 * s * rows * o.stride(0), o.stride(0), 1, cfg.dim0, cfg.P, cfg.W, 0, cfg.Tq, cfg.Tk, cfg.heads,
                     hd, 0, 0.0, None, 0, _ptr(slot), _stream()), what)
    tag_amax(o, slot)


def _attn_bwd(q, k, v, go, dq, dk, dv, cfg, packed=None):
    """packed: the [R, 2C] tensor dq and dk are the halves of (one amax slot for both, tagged on it)"""
    hd = go.shape[1] // cfg.heads
    seed = _S._cur.rng.seed_for(q.device, cfg.drop)
    sq = _new_slot(q.device)
    sk = sq if packed is not None else _new_slot(q.device)
    sv = _new_slot(q.device)
    args = (_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(go), go.stride(0),
            _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), cfg.mode, cfg.dim0,
            cfg.P, cfg.W, cfg.ws, cfg.Tq, cfg.Tk, cfg.heads, hd, cfg.mask_mode, cfg.drop.p, _ptr(seed),
            cfg.drop.salt, _ptr(sq), _ptr(sk), _ptr(sv))
    if _attn_long(cfg):      # the streaming kernels recompute the softmax statistics of every query row into a workspace
        ws, wsn = _ws(lib().npvp_attn_long_bwd_workspace_bytes(cfg.mode, cfg.dim0, cfg.P, cfg.W, cfg.ws, cfg.Tq, cfg.Tk, cfg.heads),
                      q.device)
        check(lib().npvp_attn_long_bwd(*args, _ptr(ws), wsn, _stream()), "npvp_attn_long_bwd")
    else:
        check(lib().npvp_attn_bwd(*args, _stream()), "npvp_attn_bwd")
    if packed is not None:
        tag_amax(packed, sq)
    else:
        tag_amax(dq, sq); tag_amax(dk, sk)
    tag_amax(dv, sv)


class _AttnPacked(_Function):
    """Self-attention core on a packed [R, 2C] q|k projection and a [R, C] v projection."""

    @staticmethod
    def forward(ctx, qk, v, cfg):
        remember(ctx)
        _chk(qk, v)
        C = v.shape[1]
        o = torch.empty_like(v)
        _attn_fwd(qk[:, :C], qk[:, C:], v, o, cfg)
        ctx.save_for_backward(qk, v)
        ctx.cfg = cfg
        return o

    @scoped
    def backward(ctx, go):
        qk, v = ctx.saved_tensors
        C = v.shape[1]
        go = _c(go)
        dqk, dv = torch.empty_like(qk), torch.empty_like(v)
        _attn_bwd(qk[:, :C], qk[:, C:], v, go, dqk[:, :C], dqk[:, C:], dv, ctx.cfg, packed=dqk)
        if not ctx.cfg.tiles:
            _zero_tail(ctx.cfg, dqk, dv)
        return dqk, dv, None


class _Attn(_Function):
    """Attention core with separate q [Rq,C], k [Rk,C], v [Rk,C] (the enc-dec site)."""

    @staticmethod
    def forward(ctx, q, k, v, cfg):
        remember(ctx)
        _chk(q, k, v)
        o = torch.empty_like(q)
        _attn_fwd(q, k, v, o, cfg)
        ctx.save_for_backward(q, k, v)
        ctx.cfg = cfg
        return o

    @scoped
    def backward(ctx, go):
        q, k, v = ctx.saved_tensors
        go = _c(go)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _attn_bwd(q, k, v, go, dq, dk, dv, ctx.cfg)
        return dq, dk, dv, None


def attn_packed(qk, v, cfg):
    return _AttnPacked.apply(qk, v, cfg)


def attn(q, k, v, cfg):
    return _Attn.apply(q, k, v, cfg)


def _fln_bwd(dout, h, mean, rstd, w, b, frames, PF, d, dp, T, sk, psum=None, nparts=0, want_amax=True, skip=NO_SKIP):
    """frame-LN backward (with its own statistics pass, or with the producer's `psum`); parameter gradients into the
    sink (partials reduced on the gradient stream) or returned; want_amax: dh feeds a GEMM (gets an amax slot);
    skip: the SampleSkip of the node's DropPath (`psum` form only): the frames of dropped samples are not worked on"""
    L = lib()
    dev = h.device
    dh = torch.empty_like(h)
    slot = _new_slot(dev, want_amax)
    tag_amax(dh, slot)
    dw, db = (sk[0][0], sk[1][0]) if sk else (torch.empty_like(w), torch.empty_like(b))
    ws, wsn = _ws(L.npvp_frameln_act_bwd_workspace_bytes(frames, PF), dev)
    mode = _sink_mode(sk)
    if psum is None:
        seed = _S._cur.rng.seed_for(dev, d, dp)
        check(L.npvp_frameln_act_bwd(_ptr(dout), _ptr(h), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(dh), _ptr(dw), _ptr(db),
                                     frames, PF, d.p, d.salt, dp.p, dp.salt, T, _ptr(seed), mode, _ptr(slot), _ptr(ws), wsn,
                                     _stream()), "npvp_frameln_act_bwd")
    else:
        pe = HbmProbe.begin()
        check(L.npvp_frameln_act_bwd_apply_skip(_ptr(dout), _ptr(h), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(psum), nparts,
                                                _ptr(dh), _ptr(dw), _ptr(db), frames, PF, mode, _ptr(slot), _ptr(ws), wsn, *skip.frame,
                                                _ptr(_S._cur.rng.seed_for(dev, skip.frame)), _stream()), "npvp_frameln_act_bwd_apply_skip")
        HbmProbe.end(pe, "npvp::frameln_act_bwd_fused_kernel", 4.0 * 3 * frames * PF)            # reads dout, h; writes dh
    if sk:
        _reduce_partials(sk, ws, dw, db, L.npvp_frameln_act_bwd_reduce, L.npvp_frameln_act_bwd_reduce_job, "npvp_frameln_act_bwd_reduce",
                         (frames, PF, 1), True)
        return dh, None, None
    return dh, dw, db


def _fln_pgrad(dout, h, mean, rstd, w, b, frames, PF, d, sk):
    """frame-LN backward without the input gradient (npvp_frameln_act_bwd_pgrad): -> psum [frames][PF/1024][2], dw, db
    (None, None when they went into the sink); mean / rstd are device addresses"""
    L = lib()
    dev = h.device
    psum = torch.empty(frames * (PF // 1024) * 2, dtype=torch.float32, device=dev)
    dw, db = (sk[0][0], sk[1][0]) if sk else (torch.empty_like(w), torch.empty_like(b))
    ws, wsn = _ws(L.npvp_frameln_act_bwd_workspace_bytes(frames, PF), dev)
    seed = _S._cur.rng.seed_for(dev, d)
    check(L.npvp_frameln_act_bwd_pgrad(_ptr(dout), _ptr(h), mean, rstd, _ptr(w), _ptr(b), _ptr(psum), _ptr(dw), _ptr(db),
                                       frames, PF, d.p, d.salt, 0.0, 0, 1, _ptr(seed), _sink_mode(sk), _ptr(ws), wsn, _stream()),
          "npvp_frameln_act_bwd_pgrad")
    if sk:
        _reduce_partials(sk, ws, dw, db, L.npvp_frameln_act_bwd_reduce, L.npvp_frameln_act_bwd_reduce_job, "npvp_frameln_act_bwd_reduce",
                         (frames, PF, 1), True)
        return psum, None, None
    return psum, dw, db


class _FrameLnAct(_Function):
    """out = res + droppath_n(drop(GELU(LayerNorm((Ch,H,W))(h))))   (ref VidHRFormer.py:381-382,384-386,388-390)"""

    @staticmethod
    def forward(ctx, h, w_cl, b_cl, res, frames, p_drop, p_dp, frames_per_sample, mean=None, rstd=None):
        remember(ctx)
        _chk(h, w_cl, b_cl, res)
        h = _c(h)
        PF = h.numel() // frames
        w_cl, b_cl = _c(w_cl), _c(b_cl)
        res_c = None if res is None else _c(res)
        L = lib()
        if mean is None:        # statistics not supplied by the producer of h (dwconv3x3(..., want_stats=True) emits them)
            mean = torch.empty(frames, dtype=torch.float32, device=h.device)
            rstd = torch.empty_like(mean)
            check(L.npvp_frame_stats(_ptr(h), _p(0), _ptr(mean), _ptr(rstd), frames, 1, PF, 1e-5, _stream()), "npvp_frame_stats")
        d, dp = Drop(p_drop), Drop(p_dp, 1)
        DropRecorder.note(d, "elem", h.numel())
        DropRecorder.note(dp, "group", frames // max(1, frames_per_sample))
        out = torch.empty_like(h)
        seed = _S._cur.rng.seed_for(h.device, d, dp)
        slot = _new_slot(h.device)
        check(L.npvp_frameln_act_fwd(_ptr(h), _ptr(mean), _ptr(rstd), _ptr(w_cl), _ptr(b_cl), _ptr(res_c), _ptr(out), frames,
                                     PF, d.p, d.salt, dp.p, dp.salt, frames_per_sample, _ptr(seed), _ptr(slot), _stream()),
              "npvp_frameln_act_fwd")
        tag_amax(out, slot)
        ctx.save_for_backward(h, mean, rstd, w_cl, b_cl)
        ctx.cfg = (frames, PF, d, dp, frames_per_sample, res is not None)
        ctx.sink = _ln_sink(w_cl, b_cl)
        return out

    @scoped
    def backward(ctx, dout):
        h, mean, rstd, w_cl, b_cl = ctx.saved_tensors
        frames, PF, d, dp, fps, has_res = ctx.cfg
        dout = _c(dout)
        dh, dw, db = _fln_bwd(dout, h, mean, rstd, w_cl, b_cl, frames, PF, d, dp, fps, ctx.sink)
        return dh, dw, db, (dout if has_res else None), None, None, None, None, None, None


def frameln_act(h, w_cl, b_cl, res, frames, p_drop=0.0, p_dp=0.0, frames_per_sample=1, stats=None):
    """stats = (mean, rstd) per frame when the producer of h already has them"""
    mean, rstd = stats if stats is not None else (None, None)
    return _FrameLnAct.apply(h, w_cl, b_cl, res, frames, p_drop, p_dp, frames_per_sample, mean, rstd)


class _DwConv(_Function):
    """Depthwise 3x3 on [F, H*W, Ch]; wtb = [10, Ch]: 9 tap-major weight rows + the bias row."""

    @staticmethod
    def forward(ctx, a, wtb, frames, H, W, want_stats):
        remember(ctx)
        _chk(a, wtb)
        a, wtb = _c(a), _c(wtb)
        Ch = wtb.shape[1]
        out = torch.empty_like(a)
        ctx.save_for_backward(a, wtb)
        ctx.cfg = (frames, H, W, Ch)
        if want_stats:
            mean = torch.empty(frames, dtype=torch.float32, device=a.device)
            rstd = torch.empty_like(mean)
            ws, wsn = _ws(frames * (Ch // 1024) * 8, a.device)
            check(lib().npvp_dwconv3x3_stats(_ptr(a), _ptr(wtb), _row(wtb, 9), _ptr(out), _ptr(mean), _ptr(rstd), frames, H, W,
                                             Ch, 1e-5, _ptr(ws), wsn, _stream()), "npvp_dwconv3x3_stats")
            ctx.mark_non_differentiable(mean, rstd)
            ctx.set_materialize_grads(False)
            return out, mean, rstd
        check(lib().npvp_dwconv3x3(_ptr(a), _ptr(wtb), _row(wtb, 9), _ptr(out), frames, H, W, Ch, 0, _stream()),
              "npvp_dwconv3x3")
        return out

    @scoped
    def backward(ctx, dout, *_unused):
        a, wtb = ctx.saved_tensors
        frames, H, W, Ch = ctx.cfg
        dout = _c(dout)
        L = lib()
        da = torch.empty_like(a)
        check(L.npvp_dwconv3x3(_ptr(dout), _ptr(wtb), _p(0), _ptr(da), frames, H, W, Ch, 1, _stream()), "npvp_dwconv3x3(bwd)")
        dwtb = torch.empty_like(wtb)
        ws, wsn = _ws(L.npvp_dwconv3x3_wgrad_workspace_bytes(frames, Ch), a.device)
        check(L.npvp_dwconv3x3_wgrad(_ptr(a), _ptr(dout), _ptr(dwtb), frames, H, W, Ch, _ptr(ws), wsn, _stream()),
              "npvp_dwconv3x3_wgrad")
        return da, dwtb, None, None, None, None


def dwconv3x3(a, wtb, frames, H, W, want_stats=False):
    """want_stats (8x8 grid, Ch % 1024 == 0): returns (out, mean, rstd) - the frame-LayerNorm statistics of the output"""
    return _DwConv.apply(a, wtb, frames, H, W, bool(want_stats))


class _MlpDwbn(_Function):
    """The whole conv feed-forward sub-layer body of the reference's MlpDWBN (ref/models/VidHRFormer.py:374-392) as ONE
    autograd node:  out = res + droppath(drop(GELU(norm3(fc2(drop(GELU(norm2(dw3x3(GELU(norm1(fc1(x))))))))))))
    Forward = 6 launches + 3 tiny statistics merges: fc1 GEMM (frame statistics in its epilogue) -> fused middle (norm1 +
    GELU + depthwise 3x3 + norm2's statistics: a1 is never written) -> norm2 + GELU + dropout -> fc2 GEMM (statistics) ->
    norm3 + GELU + dropout + residual + drop-path.  Backward mirrors it; the fused middle's backward recomputes a1 from h1 for
    the depthwise weight gradient and emits norm1's backward statistics, so norm1's backward is one pass.
    Passes over the [R, 2048] hidden tensor: forward 6 (was 8), backward 15 (was 18); one Python autograd node instead of 9."""

    @staticmethod
    def forward(ctx, x, res, w1, b1, n1w, n1b, dww, dwb, n2w, n2b, w2, b2, n3w, n3b, frames, T, p_drop, p_dp):
        remember(ctx)
        _chk(x, res, w1, b1, w2, b2)
        L = lib()
        R, C = x.shape
        hid, Co = w1.shape[0], w2.shape[0]
        dev, f32 = x.device, torch.float32
        st = _stream()
        PFh, PFo = 64 * hid, 64 * Co
        d2, d3, dp = Drop(p_drop), Drop(p_drop), Drop(p_dp, 1)
        # the samples dp drops: frame kernels write zeros for them, GEMM tiles inside them are not computed (DROP_PATH_SKIP) - taken in
        # forward: backward leaves out what forward left out
        ctx.skip = skip = SampleSkip.of(skip_roles("mlpdwbn", DROP_PATH_SKIP, WGRAD_ROW_SKIP), dp, T * 64, frames // max(1, T), R)
        seed = _S._cur.rng.seed_for(dev, d2, dp)
        # fc1 (+ frame statistics of h1)
        h1 = torch.empty(R, hid, dtype=f32, device=dev)
        part = torch.empty(frames * (hid // 64) * 2, dtype=f32, device=dev)
        gemm(1, 1, R, hid, C, x, x.stride(0), w1, w1.stride(0), h1, bias=b1, b_pre=_planes(w1, "F", R), rowstats=part, row_skip=skip.forward)
        stats = torch.empty(6, frames, dtype=f32, device=dev)               # mean1, rstd1, mean2, rstd2, mean3, rstd3
        # (no statistics launches: each consumer below merges the partial (mean, M2) pairs its producer left and writes
        # mean / rstd into `stats` for backward)
        # tap-major depthwise weights [9][hid] + bias row: rebuilt when the parameters changed (optimiser step / in-place update),
        # not per call (one launch per MlpDWBN and step)
        key = (WeightPlanes.epoch, dww._version, dwb._version, dww.data_ptr(), dwb.data_ptr())
        hit = dww.__dict__.get("_npvp_wtb")
        if hit is not None and hit[0] == key:
            wtb = hit[1]
        else:
            wtb = torch.empty(10, hid, dtype=f32, device=dev)
            check(L.npvp_dwtb_build(_ptr(_c(dww)), _ptr(dwb), _ptr(wtb), hid, st), "npvp_dwtb_build")
            dww.__dict__["_npvp_wtb"] = (key, wtb)
        # fused middle
        h2 = torch.empty(R, hid, dtype=f32, device=dev)
        part2 = torch.empty(frames * (hid // 512) * 2, dtype=f32, device=dev)
        check(L.npvp_mlpdw_mid_fwd_parts_skip(_ptr(h1), _ptr(part), hid // 64, 4096.0, _row(stats, 0), _row(stats, 1), _ptr(n1w),
                                              _ptr(n1b), _ptr(wtb), _row(wtb, 9), _ptr(h2), _ptr(part2), frames, 8, 8, hid, 1e-5,
                                              *skip.frame, _ptr(seed), st), "npvp_mlpdw_mid_fwd_parts_skip")
        DropRecorder.note(d2, "elem", R * hid)
        a2 = torch.empty(R, hid, dtype=f32, device=dev)
        a2_slot = _new_slot(dev)
        check(L.npvp_frameln_act_fwd_parts_skip(_ptr(h2), _ptr(part2), hid // 512, 32768.0, 1e-5, _row(stats, 2), _row(stats, 3),
                                                _ptr(n2w), _ptr(n2b), None, _ptr(a2), frames, PFh, d2.p, d2.salt, 0.0, 0, 1, _ptr(seed),
                                                _ptr(a2_slot), *skip.frame, st), "npvp_frameln_act_fwd_parts_skip")
        tag_amax(a2, a2_slot)
        # fc2 (+ statistics), norm3 + GELU + dropout + residual + drop-path
        h3 = torch.empty(R, Co, dtype=f32, device=dev)
        part3 = torch.empty(frames * (Co // 64) * 2, dtype=f32, device=dev)
        gemm(1, 1, R, Co, hid, a2, hid, w2, w2.stride(0), h3, bias=b2, b_pre=_planes(w2, "F", R), rowstats=part3, row_skip=skip.forward)
        DropRecorder.note(d3, "elem", R * Co)
        DropRecorder.note(dp, "group", frames // max(1, T))
        out = torch.empty(R, Co, dtype=f32, device=dev)
        check(L.npvp_frameln_act_fwd_parts_skip(_ptr(h3), _ptr(part3), Co // 64, 4096.0, 1e-5, _row(stats, 4), _row(stats, 5),
                                                _ptr(n3w), _ptr(n3b), _ptr(res), _ptr(out), frames, PFo, d3.p, d3.salt, dp.p, dp.salt, T,
                                                _ptr(seed), None, *skip.frame, st), "npvp_frameln_act_fwd_parts_skip")
        ctx.save_for_backward(x, h1, h2, a2, h3, stats, wtb, w1, w2, n1w, n1b, n2w, n2b, n3w, n3b)
        ctx.cfg = (frames, T, d2, d3, dp, res is not None, b1 is not None, b2 is not None)
        ctx.sinks = (_wb_sink(w1, b1), _wb_sink(w2, b2), _ln_sink(n1w, n1b), _ln_sink(n2w, n2b), _ln_sink(n3w, n3b))
        sd = _wb_sink(dww, dwb) if (dww.is_contiguous() and dwb is not None) else None
        ctx.sink_dw = sd if (sd and sd[1] is not None) else None
        return out

    @scoped
    def backward(ctx, dout):
        x, h1, h2, a2, h3, stats, wtb, w1, w2, n1w, n1b, n2w, n2b, n3w, n3b = ctx.saved_tensors
        frames, T, d2, d3, dp, has_res, has_b1, has_b2 = ctx.cfg
        s_fc1, s_fc2, s_n1, s_n2, s_n3 = ctx.sinks
        L = lib()
        R, hid = h1.shape
        Co = h3.shape[1]
        dev = x.device
        dout = _c(dout)
        dh3, gn3w, gn3b = _fln_bwd(dout, h3, stats[4], stats[5], n3w, n3b, frames, 64 * Co, d3, dp, T, s_n3)
        da2, gw2, gb2 = linear_bwd(dh3, a2, w2, True if has_b2 else None, s_fc2, skip=ctx.skip)     # (`b` only says whether there is a bias gradient to take)
        fuse_n2 = MID_BWD_N2 and hid // 16 <= 256
        if fuse_n2:
            # norm2's backward WITHOUT its input gradient: frame sums (partials) + parameter gradients in one pass over da2 / h2;
            # dh2 is evaluated inside the fused middle's backward below and never written (2 passes over [R, hidden] less)
            psum2, gn2w, gn2b = _fln_pgrad(da2, h2, _row(stats, 2), _row(stats, 3), n2w, n2b, frames, 64 * hid, d2, s_n2)
        else:
            dh2, gn2w, gn2b = _fln_bwd(da2, h2, stats[2], stats[3], n2w, n2b, frames, 64 * hid, d2, NO_DROP, 1, s_n2,
                                          want_amax=False)
            del da2
        # fused middle backward: da1, depthwise weight / bias gradient (a1 recomputed from h1), norm1's backward statistics
        da1 = torch.empty_like(h1)
        dwtb = torch.empty(10, hid, dtype=torch.float32, device=dev)
        nparts = hid // 256                     # partials per frame of norm1's backward statistics (one per block of the kernel below)
        psum = torch.empty(frames * nparts * 2, dtype=torch.float32, device=dev)
        ws, wsn = _ws(L.npvp_mlpdw_mid_bwd_workspace_bytes(frames, hid), dev)
        sk_dw = ctx.sink_dw if ctx.needs_input_grad[6] and ctx.needs_input_grad[7] else None
        wmode = 2 if sk_dw else 0          # 2: the depthwise gradient partials stay in `ws` for the gradient stream (below)
        if fuse_n2:
            seed = _S._cur.rng.seed_for(dev, d2)
            pe = HbmProbe.begin()
            check(L.npvp_mlpdw_mid_bwd_n2(_ptr(da2), _ptr(h2), _row(stats, 2), _row(stats, 3), _ptr(n2w), _ptr(n2b), _ptr(psum2),
                                          hid // 16, d2.p, d2.salt, _ptr(seed), _ptr(h1), _row(stats, 0), _row(stats, 1), _ptr(n1w),
                                          _ptr(n1b), _ptr(wtb), _ptr(da1), _ptr(dwtb), _ptr(psum), frames, 8, 8, hid, wmode, _ptr(ws), wsn,
                                          _stream()), "npvp_mlpdw_mid_bwd_n2")
            HbmProbe.end(pe, "npvp::mlpdw_mid_bwd_kernel<1, true>", 4.0 * 4 * frames * 64 * hid)     # reads da2, h2, h1; writes da1
            del da2, psum2
        else:
            check(L.npvp_mlpdw_mid_bwd(_ptr(dh2), _ptr(h1), _row(stats, 0), _row(stats, 1), _ptr(n1w), _ptr(n1b), _ptr(wtb), _ptr(da1),
                                       _ptr(dwtb), _ptr(psum), frames, 8, 8, hid, wmode, _ptr(ws), wsn, _stream()), "npvp_mlpdw_mid_bwd")
            del dh2
        if sk_dw:
            # straight into the gradient slots (on the gradient stream, like every in-place gradient write): the chunk partials
            # are reduced, transposed and accumulated by ONE launch there - no reduction on this stream, no transpose, none of
            # autograd's accumulate adds
            _reduce_partials(sk_dw, ws, sk_dw[0][0], sk_dw[1][0], L.npvp_mlpdw_mid_bwd_reduce_into, L.npvp_mlpdw_mid_bwd_reduce_job,
                             "npvp_mlpdw_mid_bwd_reduce_into", (frames, hid), False)
            gdww = gdwb = None
        else:
            gdww = torch.empty(hid, 1, 3, 3, dtype=torch.float32, device=dev)
            check(L.npvp_transpose(_ptr(dwtb), _ptr(gdww), 1, 9, hid, _stream()), "npvp_transpose")
            gdwb = dwtb[9]
        dh1, gn1w, gn1b = _fln_bwd(da1, h1, stats[0], stats[1], n1w, n1b, frames, 64 * hid, NO_DROP, NO_DROP, 1, s_n1,
                                      psum=psum, nparts=nparts, skip=ctx.skip)
        del da1
        dx, gw1, gb1 = linear_bwd(dh1, x, w1, True if has_b1 else None, s_fc1, skip=ctx.skip)
        return (dx, dout if has_res else None, gw1, gb1, gn1w, gn1b, gdww, gdwb, gn2w, gn2b, gw2, gb2, gn3w, gn3b,
                None, None, None, None)


MID_BWD_N2 = True        # (False: norm2's backward as two kernels of its own - the op test compares the two routes)
# The node leaves out work on the samples its DropPath drops: its forward frame kernels and norm1's backward write zeros for their
# frames (csrc/common.h FrameSkip) and the fc1 / fc2 forward and dgrad GEMMs run the tiles inside them on zero accumulators
# (GemmParams::rskip); the decision is taken on the device from the seed.  The fused middle's backward and norm2's parameter-gradient
# pass compute every frame (profiles/droppath_skip.txt); the weight gradients have a switch of their own, below.  False: nothing is left out (A/B runs, tests).
DROP_PATH_SKIP = True
# The fp16 weight gradients of a per-sample DropPath site - fc1 / fc2 of this node, the three projections of the spatial
# self-attention sub-layer - leave out the K-steps of dropped samples (their rows of dy are exact zeros) and deal the kept ones evenly
# over the split-K workgroups (npvp_wgrad_f16_chained_skip, and the same kernel behind npvp_gemm_f32_skip where the reduction is not
# chained: same slabs, same bits; csrc/kept_runs.h).  The kernel takes samples of at least 256 token rows, at most 64 of them; every
# other route (bf16x6, the RangeGuard fallback and strict routes, small shapes) ignores the spec.  False: every K-step runs in those
# launches (the fused dgrad + weight-gradient launch keeps the one spec DROP_PATH_SKIP gives it).  profiles/wgrad_row_skip.txt
WGRAD_ROW_SKIP = True


def mlpdwbn_fused_supported(R, C, hid, Co, H, W):
    return (GEMM_PRECISION in (4, 6) and H == 8 and W == 8 and R % 64 == 0 and hid % 512 == 0 and Co % 128 == 0 and hid % 128 == 0
            and C % 32 == 0)


def mlpdwbn(x, res, w1, b1, n1w, n1b, dww, dwb, n2w, n2b, w2, b2, n3w, n3b, frames, T, p_drop, p_dp):
    return _MlpDwbn.apply(x, res, w1, b1, n1w, n1b, dww, dwb, n2w, n2b, w2, b2, n3w, n3b, frames, T, p_drop, p_dp)


# --------------------------------------------------------------------------- sub-layer nodes
# One autograd node per residual sub-layer of a VidHRFormer block (ref/models/VidHRFormer.py:87-112,210-243): the pre-norm
# LayerNorm, the positional fuse, the projections, the attention core / FFN and the residual epilogue are a fixed sequence
# of kernel launches - nothing in between needs autograd's bookkeeping.  Against one node per kernel this removes ~3/4 of the
# Python / autograd work per step (the 8-clip shards of c3 / c4 were bound by it) and the [R, C] gradient adds autograd
# inserted where LN(x) feeds two consumers (they become the `residual` input of a dgrad GEMM's epilogue).
# The _raw_* helpers below are THE call sites of the norm entry points: the per-kernel nodes above (_LayerNorm, _LayerNormRes,
# _LayerNormNchw, _PosFuse) go through them too.
def _raw_ln_fwd(x2, w, b, eps, relu=0):
    """-> LN(x2) (+ ReLU), its statistics [2, rows] (mean, rstd)"""
    rows, C = x2.shape
    y = torch.empty_like(x2)
    st = torch.empty(2, rows, dtype=torch.float32, device=x2.device)
    slot = _new_slot(x2.device)
    check(lib().npvp_layernorm_fwd(_ptr(x2), _ptr(w), _ptr(b), _ptr(y), _row(st, 0), _row(st, 1), rows, C, eps, relu, _ptr(slot),
                                   _stream()), "npvp_layernorm_fwd")
    return tag_amax(y, slot), st


def _raw_ln_bwd(dy2, x2, w, b, st, dres, sk, relu=0, probe=False):
    """-> dx (+ dres, the residual branch's gradient), dw, db (None, None when the parameter gradients went into the sink);
    probe: the launch is one of those HbmProbe brackets (the sub-layer nodes')"""
    L = lib()
    rows, C = x2.shape
    dx = torch.empty_like(x2)
    dw, db = (sk[0][0], sk[1][0]) if sk else (torch.empty_like(w), torch.empty_like(b))
    ws, wsn = _ws(L.npvp_layernorm_bwd_workspace_bytes(rows, C), x2.device)
    slot = _new_slot(x2.device)
    pe = HbmProbe.begin() if probe else None
    check(L.npvp_layernorm_bwd(_ptr(dy2), _ptr(x2), _ptr(w), _ptr(b), _row(st, 0), _row(st, 1), _ptr(dx), _ptr(dw), _ptr(db), rows, C,
                               relu, _ptr(dres), _sink_mode(sk), _ptr(slot), _ptr(ws), wsn, _stream()), "npvp_layernorm_bwd")
    HbmProbe.end(pe, "npvp::ln_bwd_kernel<2>", 4.0 * (3 + (dres is not None)) * rows * C)            # reads dy, x (+ dres); writes dx
    tag_amax(dx, slot)
    if sk:
        _reduce_partials(sk, ws, dw, db, L.npvp_layernorm_bwd_reduce, L.npvp_layernorm_bwd_reduce_job, "npvp_layernorm_bwd_reduce",
                         (rows, C, 1), True)
        return dx, None, None
    return dx, dw, db


def _raw_posfuse_fwd(x, add, beta, gamma, N, T):
    PF = x.numel() // (N * T)
    y = torch.empty_like(x)
    st = torch.empty(2, N * T, dtype=torch.float32, device=x.device)
    slot = _new_slot(x.device)
    check(lib().npvp_posfuse_fwd(_ptr(x), _ptr(add), _ptr(beta), _ptr(gamma), _ptr(y), _row(st, 0), _row(st, 1), N, T, PF, 1e-5,
                                 _ptr(slot), _stream()), "npvp_posfuse_fwd")
    return tag_amax(y, slot), st


LN_POSFUSE_ONE_KERNEL = True          # (False: the two-kernel route, kept for the op tests)


def _raw_ln_posfuse_fwd(x2, lw, lb, eps, add, beta, gamma, N, T):
    """LayerNorm then positional fuse of its output: -> x1 = LN(x2), its statistics [2, rows], fused, its statistics [2, N*T].
    One kernel for frames of 64 token rows x 512 channels (npvp_ln_posfuse_fwd), the two-kernel route otherwise."""
    rows, C = x2.shape
    if not (LN_POSFUSE_ONE_KERNEL and C == 512 and rows == N * T * 64):
        x1, lst = _raw_ln_fwd(x2, lw, lb, eps)
        fused, pst = _raw_posfuse_fwd(x1, add, beta, gamma, N, T)
        return x1, lst, fused, pst
    x1, fused = torch.empty_like(x2), torch.empty_like(x2)
    lst = torch.empty(2, rows, dtype=torch.float32, device=x2.device)
    pst = torch.empty(2, N * T, dtype=torch.float32, device=x2.device)
    s1, s2 = _new_slot(x2.device), _new_slot(x2.device)
    check(lib().npvp_ln_posfuse_fwd(_ptr(x2), _ptr(lw), _ptr(lb), eps, _ptr(x1), _row(lst, 0), _row(lst, 1), _ptr(add), _ptr(beta),
                                    _ptr(gamma), _ptr(fused), _row(pst, 0), _row(pst, 1), N, T, 64, C, 1e-5, _ptr(s1), _ptr(s2),
                                    _stream()), "npvp_ln_posfuse_fwd")
    return tag_amax(x1, s1), lst, tag_amax(fused, s2), pst


def _raw_posfuse_bwd(dy, x, add, beta_shape, gamma, st, N, T, want_add, sinks=(None, None, None)):
    """-> du [like x], dadd, dbeta, dgamma; sinks = the ActSinks of (beta, gamma, add) where the caller found them: those gradients
    are accumulated in place and come back as None"""
    PF = x.numel() // (N * T)
    du, dbeta, dgamma = _posfuse_bwd_call(dy, x, add, gamma, st, N, T, PF, beta_shape, True, gamma is not None,
                                          sinks[0], sinks[1])
    dadd = None
    if add is not None and want_add:
        if sinks[2] is not None:
            buf, acc = sinks[2].target(add.shape, x.device)
            reduce_mid(du.view(N, T, PF), out=buf.view(N, PF), accumulate=acc)
        else:
            dadd = reduce_mid(du.view(N, T, PF)).view(add.shape)
    return du, dadd, dbeta, dgamma


# The centre-pad route of spatial window attention (cfg.grid set: the window does not tile the H x W grid; ref/models/VidHRFormer.py:
# 287-305, 488-511): the q|k and value sources are padded with zero rows BEFORE the in-projection, so a pad token's q, k, v are the bias
# vectors and it is an ordinary key of its window; the pad queries' outputs are cut away.  _raw_grid_pad / _raw_grid_cut are THE call
# sites of the two entry points; each is the other's backward.
def _raw_grid_pad(x2, cfg, want_amax=True, out=None):
    """x2 [F*H*W, C] -> [cfg.padded_rows, C]: the centre rows are x2's, every other row (border, trailing) is written as zeros.
    out: write into these rows of an existing buffer instead (x2 = None with a geometry of no frames: zero rows, _zero_tail)"""
    F_, H, W, Hp, Wp, top, left = cfg.pad_args()
    rows = cfg.padded_rows
    if out is None:
        out = torch.empty(rows, x2.shape[1], dtype=torch.float32, device=x2.device)
    C = out.shape[1]
    if (0 if x2 is None else x2.shape[0]) != F_ * H * W or (x2 is not None and x2.stride(1) != 1) or out.shape[0] != rows or out.stride(1) != 1:
        raise RuntimeError(f"grid pad: {None if x2 is None else tuple(x2.shape)} -> {tuple(out.shape)} is not {F_} frames of {H} x {W} "
                           f"unit-stride token rows -> {rows} rows")
    slot = _new_slot(out.device, want_amax)
    check(lib().npvp_grid_center_pad(_ptr(x2), C if x2 is None else x2.stride(0), _ptr(out), out.stride(0), F_, H, W, Hp, Wp, top, left, C,
                                     rows, _ptr(slot), _stream()), "npvp_grid_center_pad")
    return tag_amax(out, slot)


def _raw_grid_cut(xp, cfg, addend=None, want_amax=False):
    """xp [>= F*Hp*Wp, C] -> its centre rows [F*H*W, C] (+ addend)"""
    F_, H, W, Hp, Wp, top, left = cfg.pad_args()
    C = xp.shape[1]
    if xp.shape[0] < F_ * Hp * Wp or xp.stride(1) != 1 or (addend is not None and (addend.shape != (F_ * H * W, C) or addend.stride(1) != 1)):
        raise RuntimeError(f"grid cut: {tuple(xp.shape)} does not hold {F_} frames of {Hp} x {Wp} unit-stride token rows")
    out = torch.empty(F_ * H * W, C, dtype=torch.float32, device=xp.device)
    slot = _new_slot(xp.device, want_amax)
    check(lib().npvp_grid_center_cut(_ptr(xp), xp.stride(0), _ptr(addend), 0 if addend is None else addend.stride(0), _ptr(out),
                                     out.stride(0), F_, H, W, Hp, Wp, top, left, C, _ptr(slot), _stream()), "npvp_grid_center_cut")
    return tag_amax(out, slot)


class _ZeroRows:
    """the geometry of no frames: the pad entry point then writes `padded_rows` zero rows"""
    __slots__ = ("padded_rows",)

    def __init__(self, rows):
        self.padded_rows = rows

    def pad_args(self):
        return 0, 1, 1, 1, 1, 0, 0


def _zero_tail(cfg, *ts):
    """zero rows [F*Hp*Wp, padded_rows) of gradient buffers the attention backward filled up to F*Hp*Wp: they are rows of the
    weight- and bias-gradient GEMMs.  (A kernel, not a memset: a captured step has no memset node.  No launch when there is no tail.)"""
    body = cfg.dim0 * cfg.P
    for t in ts:
        if t.shape[0] > body:
            _raw_grid_pad(None, _ZeroRows(t.shape[0] - body), want_amax=False, out=t[body:])


class _GridPad(_Function):
    @staticmethod
    def forward(ctx, x2, cfg):
        remember(ctx)
        _chk(x2)
        ctx.cfg = cfg
        return _raw_grid_pad(_c(x2), cfg)

    @scoped
    def backward(ctx, g):
        return _raw_grid_cut(_c(g), ctx.cfg), None


class _GridCut(_Function):
    @staticmethod
    def forward(ctx, xp, cfg):
        remember(ctx)
        _chk(xp)
        ctx.cfg = cfg
        return _raw_grid_cut(_c(xp), cfg, want_amax=True)

    @scoped
    def backward(ctx, g):
        return _raw_grid_pad(_c(g), ctx.cfg), None


def grid_pad(x2, cfg):
    """token rows [F*H*W, C] -> centre-padded [cfg.padded_rows, C] (autograd: the backward is grid_cut)"""
    return _GridPad.apply(x2, cfg)


def grid_cut(xp, cfg):
    """centre-padded token rows -> [F*H*W, C] (autograd: the backward is grid_pad)"""
    return _GridCut.apply(xp, cfg)


# The learned event token of the encoder (ref/models/VidHRFormer.py:35-42, ref/models/Predictor.py:343-344): the token is appended to
# every clip as frame T+1, the positional tables get a zero frame, and the encoder's output is split into the memory (the first T
# frames) and the event coding (the last).  _raw_evt_join / _raw_evt_split are THE call sites of npvp_evt_token_join / _split; each
# is the other's backward.
def _raw_evt_join(x2, token, N, T, P, C, dev, want_amax=True):
    """x2 [N*T*P, C] (None: zeros) + token ([P, C] for all clips, [N*P, C] one per clip, None: zeros) -> [N*(T+1)*P, C]"""
    per_clip = token is not None and token.shape[0] != P
    if ((x2 is not None and (tuple(x2.shape) != (N * T * P, C) or x2.stride(1) != 1))
            or (token is not None and (tuple(token.shape) != ((N if per_clip else 1) * P, C) or not token.is_contiguous()))):
        raise RuntimeError(f"evt token join: {None if x2 is None else tuple(x2.shape)} + token {None if token is None else tuple(token.shape)} "
                           f"is not {N} clips of {T} frames of {P} unit-stride token rows of {C} and a [P, C] or [N*P, C] token")
    out = torch.empty(N * (T + 1) * P, C, dtype=torch.float32, device=dev)
    slot = _new_slot(dev, want_amax)
    check(lib().npvp_evt_token_join(_ptr(x2), C if x2 is None else x2.stride(0), _ptr(token), C, P * C if per_clip else 0, _ptr(out), C,
                                    N, T, P, C, _ptr(slot), _stream()), "npvp_evt_token_join")
    return tag_amax(out, slot)


def _raw_evt_split(y2, N, T, P, want_x=True, want_last=True, want_amax=True):
    """y2 [N*(T+1)*P, C] -> (x [N*T*P, C] or None, last [N*P, C] or None)"""
    C = y2.shape[1]
    if y2.shape[0] != N * (T + 1) * P or y2.stride(1) != 1:
        raise RuntimeError(f"evt token split: {tuple(y2.shape)} is not {N} clips of {T} + 1 frames of {P} unit-stride token rows")
    x = torch.empty(N * T * P, C, dtype=torch.float32, device=y2.device) if want_x else None
    last = torch.empty(N * P, C, dtype=torch.float32, device=y2.device) if want_last else None
    sx, sl = _new_slot(y2.device, want_amax and want_x), _new_slot(y2.device, want_amax and want_last)
    check(lib().npvp_evt_token_split(_ptr(y2), y2.stride(0), _ptr(x), C, _ptr(last), C, N, T, P, C, _ptr(sx), _ptr(sl), _stream()),
          "npvp_evt_token_split")
    return (None if x is None else tag_amax(x, sx)), (None if last is None else tag_amax(last, sl))


class _EvtJoin(_Function):
    """x (N,T,...,C) + token ((1,...,C) shared by the clips, (N,...,C) one per clip, or None: a zero frame) -> (N,T+1,...,C).
    Backward: the split; a shared token's gradient is the fixed-order sum of `last` over the clips (npvp_reduce_mid) and goes back
    through autograd, which orders the contributions of the two encoder passes of a stochastic step."""

    @staticmethod
    def forward(ctx, x, token):
        remember(ctx)
        _chk(x, token)
        N, T, C = x.shape[0], x.shape[1], x.shape[-1]
        P = x.numel() // (N * T * C)
        tk = None if token is None else _c(token).reshape(-1, C)
        ctx.geom = (N, T, P, C, None if token is None else token.shape)
        y = _raw_evt_join(_c(x).reshape(N * T * P, C), tk, N, T, P, C, x.device)
        return y.view(N, T + 1, *x.shape[2:])

    @scoped
    def backward(ctx, g):
        N, T, P, C, tshape = ctx.geom
        want_t = tshape is not None and ctx.needs_input_grad[1]
        if not (want_t or ctx.needs_input_grad[0]):
            return None, None
        dx, dlast = _raw_evt_split(_c(g).reshape(-1, C), N, T, P, ctx.needs_input_grad[0], want_t, want_amax=False)
        if want_t and tshape[0] == 1 and N > 1:
            dlast = reduce_mid(dlast.view(1, N, P * C))
        return (None if dx is None else dx.view(N, T, *g.shape[2:])), (dlast.view(tshape) if want_t else None)


class _EvtSplit(_Function):
    """y (N,T+1,...,C) -> x (N,T,...,C), last [N, P, C] (want_x False: last alone; x is then an empty tensor).  Backward: the join of
    the two gradients, an output without a gradient counting as zeros."""

    @staticmethod
    def forward(ctx, y, want_x):
        remember(ctx)
        _chk(y)
        N, T, C = y.shape[0], y.shape[1] - 1, y.shape[-1]
        P = y.numel() // (N * (T + 1) * C)
        ctx.geom = (N, T, P, C, y.shape)
        ctx.set_materialize_grads(False)
        x, last = _raw_evt_split(_c(y).reshape(-1, C), N, T, P, want_x, True)
        slot_of = lambda t: getattr(t, "_npvp_amax", (None,))[0]
        last3 = tag_amax(last.view(N, P, C), slot_of(last))
        if x is None:
            x = y.new_empty(0)
            ctx.mark_non_differentiable(x)
            return x, last3
        return tag_amax(x.view(N, T, *y.shape[2:]), slot_of(x)), last3

    @scoped
    def backward(ctx, dx, dlast):
        N, T, P, C, shape = ctx.geom
        if dx is None and dlast is None:
            return None, None
        dev = (dx if dx is not None else dlast).device
        dy = _raw_evt_join(None if dx is None else _c(dx).reshape(N * T * P, C), None if dlast is None else _c(dlast).reshape(N * P, C),
                           N, T, P, C, dev, want_amax=False)
        return dy.view(shape), None


def evt_token_join(x, token):
    """x (N,T,H,W,C) + the event token (1,H,W,C) (or one per clip (N,H,W,C), or None: zeros) -> (N,T+1,H,W,C)  (autograd: the backward
    is evt_token_split, and the sum over clips for a shared token)"""
    return _EvtJoin.apply(x, token)


def evt_token_split(y, want_x=True):
    """(N,T+1,H,W,C) -> the first T frames (N,T,H,W,C) and the last frame [N, H*W, C], each contiguous with its own amax slot
    (want_x False: the first is not produced - an empty tensor)"""
    return _EvtSplit.apply(y, want_x)


def evt_pad_table(table, T):
    """a positional table [T*P, C] -> [(T+1)*P, C] with a zero last frame (ref/models/VidHRFormer.py:40-41), a NEW tensor with its own
    ActSink: the encoder's sub-layers sum their table gradients in place into it, and its backward cuts the first T*P rows back into
    the original table's gradient.  None (fuse_method 'Add' has no gamma) stays None."""
    if table is None:
        return None
    C = table.shape[-1]
    return fan_out(_EvtJoin.apply(table.reshape(1, T, -1, C), None).view(-1, C))


class _RowTail:
    """The degenerate geometry of the two entry points: one frame, an R x 1 grid with nothing around it, followed by zero rows up to
    the next multiple of 32 - what a linear layer over R token rows needs where R is no multiple of 32 (the weight-gradient GEMM
    sums over the rows in steps of 32; zero rows add exact zeros to dW, and the cut hands zero gradient rows back, so db is
    untouched too)."""
    __slots__ = ("R", "padded_rows")

    def __init__(self, R):
        self.R, self.padded_rows = R, -(-R // 32) * 32

    def pad_args(self):
        return 1, self.R, 1, self.R, 1, 0, 0


def linear_any_rows(x, w, b=None):
    """ops.linear for any number of token rows: zero rows are appended to the input and cut from the output where the count is no
    multiple of 32 (a 6 x 10 grid's NRMLP tables and event-coding rows); the same call as ops.linear where it is"""
    if x.shape[0] % 32 == 0:
        return linear(x, w, b)
    tail = _RowTail(x.shape[0])
    return grid_cut(linear(grid_pad(x, tail), w, b), tail)


class _SelfAttnSublayer(_Function):
    """y = x + drop(out_proj(attn(q = k = fuse(LN(x) [+ add]), v = LN(x))))   - spatial-window or temporal self-attention
    (ref/models/VidHRFormer.py:87-88,94-107,210-212,217-221): LN, positional fuse (2 kernels), q|k GEMM, v GEMM, attention
    core, out-projection GEMM with the dropout / drop-path + residual epilogue."""

    @staticmethod
    def forward(ctx, x, lw, lb, eps, beta, gamma, add, wqk, bqk, wv, bv, wo, bo, cfg, drop, N, T):
        remember(ctx)
        # wqk / wv are the [:2C] / [2C:] row slices of in_proj_weight, sliced by the caller WITH grad mode on: a slice taken in
        # here (grad mode off) would not be recognised as a view of a flat-buffer parameter by GradSink
        _chk(x, lw, lb, beta, gamma, add, wqk, bqk, wv, bv, wo, bo)
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        beta_c = _c(beta)
        gamma_c = None if gamma is None else _c(gamma)
        add_c = None if add is None else _c(add)
        x1, lst, fused, pst = _raw_ln_posfuse_fwd(x2, lw, lb, eps, add_c, beta_c, gamma_c, N, T)
        if cfg.tiles:
            qk = linear_fwd(fused, wqk, bqk)
            v = linear_fwd(x1, wv, bv)
            o = torch.empty_like(v)
            _attn_fwd(qk[:, :C], qk[:, C:], v, o, cfg)
        else:
            # centre-pad route: both projections and the core run on the padded rows (a zero row projects to the bias), the
            # out-projection on the real rows.  The padded q|k source is saved IN PLACE of the unpadded one (only the weight
            # gradient reads it); the padded value source is made again in the backward (x1 itself is needed there anyway)
            fused = _raw_grid_pad(fused, cfg)
            qk = linear_fwd(fused, wqk, bqk)
            v = linear_fwd(_raw_grid_pad(x1, cfg), wv, bv)
            o_p = torch.empty_like(v)
            _attn_fwd(qk[:, :C], qk[:, C:], v, o_p, cfg)
            o = _raw_grid_cut(o_p, cfg, want_amax=True)
        y = linear_fwd(o, wo, bo, residual=x2, drop=drop)
        ctx.save_for_backward(x2, x1, lst, fused, pst, qk, v, o, lw, lb, gamma_c, add_c, wqk, bqk, wv, bv, wo, bo)
        ctx.act_sinks = (ActSink.of(beta), ActSink.of(gamma), ActSink.of(add))
        ctx.cfg = (cfg, drop, N, T, x.shape, beta.shape)
        ctx.sinks = (_ln_sink(lw, lb), _wb_sink(wqk, bqk), _wb_sink(wv, bv), _wb_sink(wo, bo))
        return y.view(x.shape)

    @scoped
    def backward(ctx, dy):
        x2, x1, lst, fused, pst, qk, v, o, lw, lb, gamma, add, wqk, bqk, wv, bv, wo, bo = ctx.saved_tensors
        cfg, drop, N, T, xshape, beta_shape = ctx.cfg
        s_ln, s_qk, s_v, s_o = ctx.sinks
        C = x2.shape[1]
        dy2 = _c(dy).reshape(-1, C)
        dz, ad = masked_grad(dy2, drop, wo)
        # a per-sample DropPath (the spatial site) leaves dz - masked here or inside the GEMMs -, hence do, dqk and dv (attention stays inside a
        # sample) zero in the rows of dropped samples: the three weight gradients leave them out (WGRAD_ROW_SKIP).  The tiling route only: the
        # centre-pad route's projections run on padded rows, where the samples are no row groups
        skip = SampleSkip.of(skip_roles("self_attn", DROP_PATH_SKIP, WGRAD_ROW_SKIP), drop, drop.g1, drop.g2, dy2.shape[0]) if cfg.tiles else NO_SKIP
        do, gwo, gbo = linear_bwd(dz, o, wo, bo, s_o, a_drop=ad, skip=skip)
        if not cfg.tiles:
            do = _raw_grid_pad(do, cfg, want_amax=False)            # the pad queries' outputs were cut away: their gradient is 0
        dqk, dv = torch.empty_like(qk), torch.empty_like(v)
        _attn_bwd(qk[:, :C], qk[:, C:], v, do, dqk[:, :C], dqk[:, C:], dv, cfg, packed=dqk)
        if not cfg.tiles:
            _zero_tail(cfg, dqk, dv)
        # (centre-pad route: `fused` holds the padded rows, see forward - the bias gradients sum the pad rows too, they are keys of
        # their windows, and the weight gradients see their zero rows)
        dfused, gwqk, gbqk = linear_bwd(dqk, fused, wqk, bqk, s_qk, skip=skip)
        if not cfg.tiles:
            dfused = _raw_grid_cut(dfused, cfg)
        du, dadd, dbeta, dgamma = _raw_posfuse_bwd(dfused, x1, add, beta_shape, gamma, pst, N, T, ctx.needs_input_grad[6], ctx.act_sinks)
        if cfg.tiles:
            # dx1 = dv Wv + du: the second consumer's gradient rides in as the dgrad GEMM's residual input (no separate add)
            dx1, gwv, gbv = linear_bwd(dv, x1, wv, bv, s_v, residual=du, skip=skip)
        else:
            dx1, gwv, gbv = linear_bwd(dv, _raw_grid_pad(x1, cfg), wv, bv, s_v)
            dx1 = _raw_grid_cut(dx1, cfg, addend=du)                # ... here the shapes differ: du rides in as the cut's addend
        dx, glw, glb = _raw_ln_bwd(dx1, x2, lw, lb, lst, dy2, s_ln, probe=True)
        return (dx.view(xshape), glw, glb, None, dbeta, dgamma, dadd, gwqk, gbqk, gwv, gbv, gwo, gbo, None, None, None, None)


class _CrossAttnSublayer(_Function):
    """y = x + droppath_t(out_proj(attn(q = fuse(LN(x) + add), k = key, v = memory)))   - the decoder's encoder-decoder
    attention (ref/models/VidHRFormer.py:229-239); key = fuse(memory) is layer invariant and supplied by the caller."""

    @staticmethod
    def forward(ctx, x, lw, lb, eps, beta, gamma, add, key, memory, wq, bq, wk, bk, wv, bv, wo, bo, cfg, drop, N, T):
        remember(ctx)
        _chk(x, lw, lb, beta, gamma, add, key, memory, wq, bq, wk, bk, wv, bv, wo, bo)
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        k2, m2 = _c(key).reshape(-1, C), _c(memory).reshape(-1, C)
        beta_c = _c(beta)
        gamma_c = None if gamma is None else _c(gamma)
        add_c = None if add is None else _c(add)
        x1, lst, query, pst = _raw_ln_posfuse_fwd(x2, lw, lb, eps, add_c, beta_c, gamma_c, N, T)
        q = linear_fwd(query, wq, bq)
        k = linear_fwd(k2, wk, bk)
        v = linear_fwd(m2, wv, bv)
        o = torch.empty_like(q)
        _attn_fwd(q, k, v, o, cfg)
        y = linear_fwd(o, wo, bo, residual=x2, drop=drop)
        ctx.save_for_backward(x2, x1, lst, query, pst, q, k, v, o, k2, m2, lw, lb, gamma_c, add_c, wq, bq, wk, bk, wv, bv, wo, bo)
        ctx.act_sinks = (ActSink.of(beta), ActSink.of(gamma), ActSink.of(add))
        ctx.km_sinks = (ActSink.of(key), ActSink.of(memory))
        ctx.cfg = (cfg, drop, N, T, x.shape, beta.shape, key.shape, memory.shape)
        ctx.sinks = (_ln_sink(lw, lb), _wb_sink(wq, bq), _wb_sink(wk, bk), _wb_sink(wv, bv), _wb_sink(wo, bo))
        return y.view(x.shape)

    @scoped
    def backward(ctx, dy):
        x2, x1, lst, query, pst, q, k, v, o, k2, m2, lw, lb, gamma, add, wq, bq, wk, bk, wv, bv, wo, bo = ctx.saved_tensors
        cfg, drop, N, T, xshape, beta_shape, kshape, mshape = ctx.cfg
        s_ln, s_q, s_k, s_v, s_o = ctx.sinks
        C = x2.shape[1]
        dy2 = _c(dy).reshape(-1, C)
        dz, ad = masked_grad(dy2, drop, wo)
        do, gwo, gbo = linear_bwd(dz, o, wo, bo, s_o, a_drop=ad)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _attn_bwd(q, k, v, do, dq, dk, dv, cfg)
        dquery, *gq = linear_bwd(dq, query, wq, bq, s_q)
        du, dadd, dbeta, dgamma = _raw_posfuse_bwd(dquery, x1, add, beta_shape, gamma, pst, N, T, ctx.needs_input_grad[6], ctx.act_sinks)
        dkey = dmem = None
        for need, g_, w_, sink, shape, which in ((ctx.needs_input_grad[7], dk, wk, ctx.km_sinks[0], kshape, 0),
                                                 (ctx.needs_input_grad[8], dv, wv, ctx.km_sinks[1], mshape, 1)):
            if not need:
                continue
            if sink is not None:        # the decoder's 8 layers share key / memory: their gradients are summed by the dgrad GEMMs' epilogues
                buf, acc = sink.target(shape, g_.device)
                linear_dgrad(g_, w_, out=buf.view(g_.shape[0], C), accumulate=acc)
            elif which == 0:
                dkey = linear_dgrad(g_, w_).view(shape)
            else:
                dmem = linear_dgrad(g_, w_).view(shape)
        gk = _lin_grads(dk, k2, wk, bk, s_k)
        gv = _lin_grads(dv, m2, wv, bv, s_v)
        dx, glw, glb = _raw_ln_bwd(du, x2, lw, lb, lst, dy2, s_ln, probe=True)
        return (dx.view(xshape), glw, glb, None, dbeta, dgamma, dadd, dkey, dmem, gq[0], gq[1], gk[0], gk[1], gv[0], gv[1], gwo, gbo,
                None, None, None, None)


class _FfnSublayer(_Function):
    """y = x + drop3(linear2(drop2(GELU(linear1(LN(x))))))   (ref/models/VidHRFormer.py:110-112,224-226)"""

    @staticmethod
    def forward(ctx, x, lw, lb, eps, w1, b1, w2, b2, p):
        remember(ctx)
        _chk(x, lw, lb, w1, b1, w2, b2)
        C = x.shape[-1]
        x2 = _c(x).reshape(-1, C)
        xn, lst = _raw_ln_fwd(x2, lw, lb, eps)
        h, a, y, d2, d3 = _ffn_fwd(xn, x2, w1, b1, w2, b2, p)
        ctx.save_for_backward(x2, xn, lst, h, a, lw, lb, w1, b1, w2, b2)
        ctx.cfg = (d2, d3, x.shape)
        ctx.sinks = (_ln_sink(lw, lb), _wb_sink(w1, b1), _wb_sink(w2, b2))
        return y.view(x.shape)

    @scoped
    def backward(ctx, dy):
        x2, xn, lst, h, a, lw, lb, w1, b1, w2, b2 = ctx.saved_tensors
        d2, d3, xshape = ctx.cfg
        s_ln, s1, s2 = ctx.sinks
        C = x2.shape[1]
        dy2 = _c(dy).reshape(-1, C)
        dz2, ad = masked_grad(dy2, d3, w2)
        dh_slot = _new_slot(dy2.device)
        dh, gw2, gb2 = linear_bwd(dz2, a, w2, b2, s2, act=3, aux_in=h, drop=d2, dx_amax=dh_slot, a_drop=ad)
        tag_amax(dh, dh_slot)
        dxn, gw1, gb1 = linear_bwd(dh, xn, w1, b1, s1)
        dx, glw, glb = _raw_ln_bwd(dxn, x2, lw, lb, lst, dy2, s_ln, probe=True)
        return dx.view(xshape), glw, glb, None, gw1, gb1, gw2, gb2, None


def self_attn_sublayer(x, norm, beta, gamma, add, mha, cfg, drop, N, T):
    C = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    return _SelfAttnSublayer.apply(x, norm.weight, norm.bias, norm.eps, beta, gamma, add, w[:2 * C], b[:2 * C], w[2 * C:], b[2 * C:],
                                   mha.out_proj.weight, mha.out_proj.bias, cfg, drop, N, T)


def cross_attn_sublayer(x, norm, beta, gamma, add, key, memory, mha, cfg, drop, N, T):
    C = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    return _CrossAttnSublayer.apply(x, norm.weight, norm.bias, norm.eps, beta, gamma, add, key, memory, w[:C], b[:C], w[C:2 * C],
                                    b[C:2 * C], w[2 * C:], b[2 * C:], mha.out_proj.weight, mha.out_proj.bias, cfg, drop, N, T)


def _no_grad_inputs(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{what} is forward only: call it under torch.no_grad() or on tensors that do not require grad")


def cross_attn_samples(x, norm, beta, gamma, add, key, memory, mha, cfg, S, N, T):
    """The encoder-decoder sub-layer of the sampler (forward only): the arithmetic of _CrossAttnSublayer.forward with `drop` off for
    x of S * N clips (sample-major) and add [S * N, H, W, C], against key / memory of N clips.  LN + positional fuse + Q projection
    run on the S * N clips, the K and V projections on the N clips, the core is _attn_samples_fwd (cfg: the N-clip temporal
    configuration, cfg.dim0 == N), then the out-projection with the residual."""
    w, b = mha.in_proj_weight, mha.in_proj_bias
    _no_grad_inputs("cross_attn_samples", x, add, key, memory, beta, gamma, w, b, mha.out_proj.weight, mha.out_proj.bias, norm.weight, norm.bias)
    _chk(x, beta, gamma, add, key, memory, w, b)
    if cfg.dim0 != N or x.shape[0] != S * N:
        raise ValueError(f"cross_attn_samples: x must hold S * N = {S * N} clips and cfg the N = {N} clips of the memory")
    C = mha.embed_dim
    with torch.no_grad():
        x2 = _c(x).reshape(-1, C)
        k2, m2 = _c(key).reshape(-1, C), _c(memory).reshape(-1, C)
        _, _, query, _ = _raw_ln_posfuse_fwd(x2, norm.weight, norm.bias, norm.eps, None if add is None else _c(add), _c(beta),
                                             None if gamma is None else _c(gamma), S * N, T)
        q = linear_fwd(query, w[:C], b[:C])
        k = linear_fwd(k2, w[C:2 * C], b[C:2 * C])
        v = linear_fwd(m2, w[2 * C:], b[2 * C:])
        o = torch.empty_like(q)
        _attn_samples_fwd(q, k, v, o, cfg, S)
        y = linear_fwd(o, mha.out_proj.weight, mha.out_proj.bias, residual=x2)
    return y.view(x.shape)


def reparam_samples(mu, logvar, S, seed, salt, sample_base=0, return_eps=False):
    """S draws of z = mu + exp(0.5 logvar) * eps (ref/models/submodules.py:408-410) in one launch: -> z [S, *mu.shape] (and eps, same
    shape).  eps is Box-Muller over the library's counter hash of (seed, salt, element index in the array of ALL samples): sample
    sample_base + s has the same bits for every S and every split of S into calls (csrc/sample.hip has the formula).  seed: a
    one-element int64 DEVICE tensor (the scheduling context's seed tensor, or one of the caller's); salt: an int below 2^32."""
    _no_grad_inputs("reparam_samples", mu, logvar)
    _chk(mu, logvar)
    if mu.shape != logvar.shape:
        raise ValueError("reparam_samples: mu and logvar must have one shape")
    if not (seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise ValueError("reparam_samples: seed must be a one-element int64 tensor on the device")
    mu_c, lv_c = _c(mu.detach()), _c(logvar.detach())
    z = torch.empty((S,) + tuple(mu.shape), dtype=torch.float32, device=mu.device)
    eps = torch.empty_like(z) if return_eps else None
    check(lib().npvp_reparam_samples(_ptr(mu_c), _ptr(lv_c), _ptr(z), _ptr(eps), mu_c.numel(), S, sample_base, _ptr(seed),
                                     int(salt) & 0xFFFFFFFF, _stream()), "npvp_reparam_samples")
    return (z, eps) if return_eps else z


def ffn_sublayer(x, norm, lin1, lin2, p):
    return _FfnSublayer.apply(x, norm.weight, norm.bias, norm.eps, lin1.weight, lin1.bias, lin2.weight, lin2.bias, p)


class _Im2Col(_Function):
    """[F, H*W, C] -> [F*H*W, 9*C] patches of a 3x3 / pad-1 conv (tap-major columns); backward = col2im."""

    @staticmethod
    def forward(ctx, x, frames, H, W):
        remember(ctx)
        _chk(x)
        x = _c(x)
        C = x.shape[-1]
        out = torch.empty(frames * H * W, 9 * C, dtype=torch.float32, device=x.device)
        check(lib().npvp_im2col3x3(_ptr(x), _ptr(out), frames, H, W, C, 0, _stream()), "npvp_im2col3x3")
        ctx.cfg = (frames, H, W, C, x.shape)
        return out

    @scoped
    def backward(ctx, g):
        frames, H, W, C, shape = ctx.cfg
        g = _c(g)
        out = torch.empty(shape, dtype=torch.float32, device=g.device)
        check(lib().npvp_im2col3x3(_ptr(g), _ptr(out), frames, H, W, C, 1, _stream()), "npvp_im2col3x3(col2im)")
        return out, None, None, None


def im2col3x3(x, frames, H, W):
    return _Im2Col.apply(x, frames, H, W)


def nchw_to_canonical(x):
    """(N,T,C,H,W) -> canonical [N*T, H*W, C].  A channels-last feature tensor (what the frozen encoder emits when it
    runs in torch.channels_last) already IS the canonical layout: it is viewed, not transposed."""
    if x.dim() == 5 and x.permute(0, 1, 3, 4, 2).is_contiguous() and not x.requires_grad:
        N, T, C, H, W = x.shape
        return x.permute(0, 1, 3, 4, 2).reshape(N * T, H * W, C)
    return _nchw_to_canonical(x)


def _nchw_to_canonical(x):
    """(N,T,C,H,W) -> canonical [N*T, H*W, C]"""
    N, T, C, H, W = x.shape
    return _Transpose.apply(x.reshape(N * T, C, H * W))


def canonical_to_nchw(x, N, T, H, W):
    """[N*T, H*W, C] -> (N,T,C,H,W)"""
    C = x.shape[-1]
    return _Transpose.apply(x.reshape(N * T, H * W, C)).reshape(N, T, C, H, W)


def mean_mid(x):
    return _MeanMid.apply(x)


# --------------------------------------------------------------------------- frozen autoencoder epilogues (csrc/ae.hip)
def _nchw_layout(x, what):
    """(x, outer, inner, layout) of an (N,C,H,W) tensor as the layout kernels read it: channels_last memory is layout 0 (rows
    [N*H*W][C]), contiguous memory layout 1 (planes [N*C][H*W]); anything else is made contiguous first"""
    if x.dim() != 4:
        raise RuntimeError(f"{what}: x must be (N, C, H, W)")
    N, C, H, W = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        return x, N * H * W, C, 0
    return x.contiguous(), N * C, H * W, 1


def _memory_format(layout):
    return torch.channels_last if layout == 0 else torch.contiguous_format


class _BiasAct(_Function):
    """out = act(x + bias[c]) (+ residual) on an (N,C,H,W) tensor in contiguous or channels_last memory; bias is frozen.
    Gradient w.r.t. x only (the decoder's input-gradient path), through the saved OUTPUT."""

    @staticmethod
    def forward(ctx, x, bias, residual, act):
        remember(ctx)
        _chk(x, bias, residual)
        need_x, need_res = ctx.needs_input_grad[0], ctx.needs_input_grad[2]     # (read before x may be rebound to a no-grad copy)
        x, outer, inner, layout = _nchw_layout(x, "bias_act")
        if residual is not None and residual.stride() != x.stride():
            residual = residual.contiguous(memory_format=_memory_format(layout))
        out = torch.empty_like(x)
        check(lib().npvp_bias_act(_ptr(x), _ptr(bias), _ptr(residual), _ptr(out), outer, inner, x.shape[1], layout, act, _stream()),
              "npvp_bias_act")
        ctx.act, ctx.cl, ctx.has_res = act, layout == 0, residual is not None
        if need_x or need_res:
            if residual is not None:
                raise NotImplementedError("bias_act: backward with a fused skip-add is not on the Stage-2 path")
            ctx.save_for_backward(out)
        return out

    @scoped
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.contiguous(memory_format=torch.channels_last if ctx.cl else torch.contiguous_format)
        dx = torch.empty_like(y)
        check(lib().npvp_act_bwd(_ptr(g), _ptr(y), _ptr(dx), y.numel(), ctx.act, _stream()), "npvp_act_bwd")
        return dx, None, None, None


def bias_act(x, bias, act=0, residual=None):
    return _BiasAct.apply(x, bias, residual, act)


def bias_act_scaled(x, bias, scale, act=0, residual=None):
    """out = residual + s * act(x + bias[c]) on an (N,C,H,W) tensor in contiguous or channels_last memory, one pass
    (npvp_bias_act_scaled): the tail of the frozen NonLocalAttenion2D.  scale: a one-element DEVICE tensor the kernel reads (no
    .item(), no host synchronisation), or None for s = 1.  Forward only: an input that requires grad is refused."""
    ts = [t for t in (x, bias, scale, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise NotImplementedError("bias_act_scaled: forward only (the frozen autoencoder's attention tail); an input requires grad")
    _chk(*ts)
    if x.dim() != 4 or bias.shape != (x.shape[1],):
        raise RuntimeError("bias_act_scaled: x must be (N, C, H, W) and bias (C,)")
    if scale is not None and scale.numel() != 1:
        raise RuntimeError("bias_act_scaled: scale must hold one float")
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError("bias_act_scaled: residual shape differs from x")
    x, outer, inner, layout = _nchw_layout(x, "bias_act_scaled")
    if residual is not None and residual.stride() != x.stride():
        residual = residual.contiguous(memory_format=_memory_format(layout))
    out = torch.empty_like(x)
    bias = _c(bias)
    check(lib().npvp_bias_act_scaled(_ptr(x), _ptr(bias), _ptr(scale), _ptr(residual), _ptr(out), outer, inner, x.shape[1], layout, act,
                                     _stream()), "npvp_bias_act_scaled")
    return out


# --------------------------------------------------------------------------- frozen encoder: 3 x 3 convolutions on the MFMA (csrc/conv3x3.hip)
CONV3X3_PAD = {"zero": 0, "reflect": 1}


def conv3x3_takes(C_in, C_out):
    """channel counts the 3 x 3 implicit-GEMM kernel is built for"""
    return C_in > 0 and C_out > 0 and C_in % 64 == 0 and C_out % 64 == 0


def conv3x3_planes(w):
    """(planes, w_amax) of a frozen weight w [C_out][C_in][3][3]: the scaled two-term fp16 planes npvp_conv3x3_f16 reads, K ordered
    (kh, kw, ci), and the weight's amax slot as a 512-float tensor (a plain buffer: it lives as long as the module that holds it)"""
    _chk(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not conv3x3_takes(w.shape[1], w.shape[0]):
        raise RuntimeError("conv3x3_planes: w must be [C_out][C_in][3][3] with channel counts that are multiples of 64")
    w = w.detach().contiguous()
    C_out, C_in = w.shape[:2]
    planes = torch.empty(lib().npvp_conv3x3_planes_bytes(C_in, C_out) // 2, dtype=torch.float16, device=w.device)
    slot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(lib().npvp_conv3x3_planes(_ptr(w), C_in, C_out, _ptr(planes), _ptr(slot), _stream()), "npvp_conv3x3_planes")
    return planes, slot


def conv3x3_packed(x, planes, w_amax, bias, pad="zero", act=0, residual=None, want_amax=True):
    """y = act(conv3x3(x) + bias[c]) (+ residual) of a frozen 3 x 3 stride-1 "same" convolution on channels-last frames x (F, C_in, H, W),
    one npvp_conv3x3_f16 launch (f16x3 implicit GEMM: no padded copy, no im2col tensor, no separate epilogue pass).  planes / w_amax:
    conv3x3_planes of the folded weight; pad: "zero" or "reflect" (ReflectionPad2d(1)).  The amax slot of x is its producer's or one
    npvp_amax pass (amax_of); want_amax attaches the slot of y to the result, so a following convolution needs no pass.
    Forward only: an input that requires grad is refused.  x and residual must be channels-last (no silent copy)."""
    ts = [t for t in (x, bias, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise NotImplementedError("conv3x3_packed: forward only (the frozen encoder's convolutions); an input requires grad")
    _chk(x, w_amax, bias, residual)
    if x.dim() != 4:
        raise RuntimeError("conv3x3_packed: x must be (F, C_in, H, W)")
    Fr, C_in, H, W = x.shape
    C_out = bias.shape[0]
    if planes.numel() != 2 * 9 * C_in * C_out or not planes.is_cuda or planes.dtype != torch.float16:
        raise RuntimeError("conv3x3_packed: planes do not belong to a [C_out][C_in][3][3] weight of these channel counts")
    x2 = x.permute(0, 2, 3, 1)
    if not x2.is_contiguous():
        raise RuntimeError("conv3x3_packed: x must be channels-last")
    y = torch.empty((Fr, H, W, C_out), device=x.device, dtype=torch.float32)
    if residual is not None:
        if residual.shape != (Fr, C_out, H, W) or not residual.permute(0, 2, 3, 1).is_contiguous():
            raise RuntimeError("conv3x3_packed: residual must be channels-last frames of the output's shape")
    x_slot = amax_of(x2.reshape(Fr * H * W, C_in))                  # (a view of x: finds the slot its producer attached to x)
    y_slot = AmaxSlot.new(x.device) if want_amax else None
    check(lib().npvp_conv3x3_f16(_ptr(x), _ptr(planes), _ptr(_c(bias)), _ptr(residual), _ptr(y), Fr, H, W, C_in, C_out, CONV3X3_PAD[pad], act,
                                 _ptr(x_slot), _ptr(w_amax), _ptr(y_slot), None, 0, _stream()), "npvp_conv3x3_f16")
    tag_amax(y, y_slot)                                             # (amax_of looks at a view's base)
    return tag_amax(y.permute(0, 3, 1, 2), y_slot)


def conv3x3s2_takes(C_in, C_out):
    """channel counts the stride-2 form of the kernel is built for (C_in = 32: block1 of the ngf = 32 encoders)"""
    return C_in > 0 and C_out > 0 and C_in % 32 == 0 and C_out % 64 == 0


def conv3x3s2_planes(w):
    """conv3x3_planes under the stride-2 channel rule (conv3x3s2_takes): (planes, w_amax) of a frozen weight w [C_out][C_in][3][3] in
    the same layout, for conv3x3s2_packed"""
    _chk(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not conv3x3s2_takes(w.shape[1], w.shape[0]):
        raise RuntimeError("conv3x3s2_planes: w must be [C_out][C_in][3][3] with C_in a multiple of 32 and C_out a multiple of 64")
    w = w.detach().contiguous()
    C_out, C_in = w.shape[:2]
    planes = torch.empty(lib().npvp_conv3x3s2_planes_bytes(C_in, C_out) // 2, dtype=torch.float16, device=w.device)
    slot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(lib().npvp_conv3x3s2_planes(_ptr(w), C_in, C_out, _ptr(planes), _ptr(slot), _stream()), "npvp_conv3x3s2_planes")
    return planes, slot


def conv3x3s2_packed(x, planes, w_amax, bias, act=0, residual=None, want_amax=True):
    """y = act(conv3x3(x, stride 2, zero padding 1) + bias[c]) (+ residual) of a frozen downsampling convolution on channels-last frames
    x (F, C_in, H, W) -> (F, C_out, (H + 1) // 2, (W + 1) // 2), one npvp_conv3x3s2_f16 launch (the stride-2 form of conv3x3_packed's
    kernel).  planes / w_amax: conv3x3s2_planes of the folded weight.  The amax slot of x is its producer's or one npvp_amax pass
    (amax_of); want_amax attaches the slot of y to the result and to its NCHW view, so a following conv3x3_packed needs no pass.
    Forward only: an input that requires grad is refused.  x and residual must be channels-last (no silent copy)."""
    ts = [t for t in (x, bias, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise NotImplementedError("conv3x3s2_packed: forward only (the frozen encoder's convolutions); an input requires grad")
    _chk(x, w_amax, bias, residual)
    if x.dim() != 4:
        raise RuntimeError("conv3x3s2_packed: x must be (F, C_in, H, W)")
    Fr, C_in, H, W = x.shape
    C_out = bias.shape[0]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if planes.numel() != 2 * 9 * C_in * C_out or not planes.is_cuda or planes.dtype != torch.float16:
        raise RuntimeError("conv3x3s2_packed: planes do not belong to a [C_out][C_in][3][3] weight of these channel counts")
    x2 = x.permute(0, 2, 3, 1)
    if not x2.is_contiguous():
        raise RuntimeError("conv3x3s2_packed: x must be channels-last")
    y = torch.empty((Fr, Ho, Wo, C_out), device=x.device, dtype=torch.float32)
    if residual is not None:
        if residual.shape != (Fr, C_out, Ho, Wo) or not residual.permute(0, 2, 3, 1).is_contiguous():
            raise RuntimeError("conv3x3s2_packed: residual must be channels-last frames of the output's shape")
    x_slot = amax_of(x2.reshape(Fr * H * W, C_in))                  # (a view of x: finds the slot its producer attached to x)
    y_slot = AmaxSlot.new(x.device) if want_amax else None
    check(lib().npvp_conv3x3s2_f16(_ptr(x), _ptr(planes), _ptr(_c(bias)), _ptr(residual), _ptr(y), Fr, H, W, C_in, C_out, act, _ptr(x_slot),
                                   _ptr(w_amax), _ptr(y_slot), None, 0, _stream()), "npvp_conv3x3s2_f16")
    tag_amax(y, y_slot)
    return tag_amax(y.permute(0, 3, 1, 2), y_slot)


# --------------------------------------------------------------------------- frozen decoder: transposed 3 x 3 convolutions (csrc/conv3x3.hip)
def convt3x3s2_takes(C_in, C_out):
    """channel counts of a ConvTranspose2d(3, stride 2, padding 1, output_padding 1) the route runs: the forward kernel needs
    C_out % 64 == 0, the input gradient is npvp_conv3x3s2_f16 with in = C_out, out = C_in and needs C_in % 64 == 0"""
    return C_in > 0 and C_out > 0 and C_in % 64 == 0 and C_out % 64 == 0


ConvT3x3Planes = namedtuple("ConvT3x3Planes", "fwd w_amax bwd bwd_w_amax zero_bias")


def convt3x3s2_planes(w):
    """the planes of a frozen ConvTranspose2d weight w [C_in][C_out][3][3] for convt3x3s2_packed: (fwd, w_amax) for the forward kernel
    (npvp_convt3x3s2_planes), (bwd, bwd_w_amax) for the input gradient - npvp_conv3x3s2_planes on the SAME weight memory read as a
    Conv2d weight [out = C_in][in = C_out][3][3] - and the zero bias of C_in floats that launch takes"""
    _chk(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not convt3x3s2_takes(w.shape[0], w.shape[1]):
        raise RuntimeError("convt3x3s2_planes: w must be [C_in][C_out][3][3] with channel counts that are multiples of 64")
    w = w.detach().contiguous()
    C_in, C_out = w.shape[:2]
    L = lib()
    fwd = torch.empty(L.npvp_convt3x3s2_planes_bytes(C_in, C_out) // 2, dtype=torch.float16, device=w.device)
    slot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(L.npvp_convt3x3s2_planes(_ptr(w), C_in, C_out, _ptr(fwd), _ptr(slot), _stream()), "npvp_convt3x3s2_planes")
    bwd = torch.empty(L.npvp_conv3x3s2_planes_bytes(C_out, C_in) // 2, dtype=torch.float16, device=w.device)
    bslot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(L.npvp_conv3x3s2_planes(_ptr(w), C_out, C_in, _ptr(bwd), _ptr(bslot), _stream()), "npvp_conv3x3s2_planes")
    return ConvT3x3Planes(fwd, slot, bwd, bslot, torch.zeros(C_in, device=w.device))


class _ConvT3x3S2(_Function):
    """y = act(conv_transpose3x3(x, stride 2, padding 1, output_padding 1) + bias[c]) of a frozen weight, channels-last.  Gradient
    w.r.t. x only (the decoder's input-gradient path): dx = conv3x3(act'(y) g, stride 2, padding 1) with the weight read as a Conv2d
    weight - npvp_act_bwd through the saved OUTPUT, one npvp_amax pass, the existing npvp_conv3x3s2_f16."""

    @staticmethod
    def forward(ctx, x, bias, act, fwd, w_amax, bwd, bwd_w_amax, zero_bias):
        remember(ctx)
        Fr, C_in, H, W = x.shape
        C_out = bias.shape[0]
        x2 = x.permute(0, 2, 3, 1)
        y = torch.empty((Fr, 2 * H, 2 * W, C_out), device=x.device, dtype=torch.float32)
        x_slot = amax_of(x2.reshape(Fr * H * W, C_in))                  # (a view of x: finds the slot its producer attached to x)
        y_slot = AmaxSlot.new(x.device)
        check(lib().npvp_convt3x3s2_f16(_ptr(x), _ptr(fwd), _ptr(bias), _ptr(y), Fr, H, W, C_in, C_out, act, _ptr(x_slot), _ptr(w_amax),
                                        _ptr(y_slot), None, 0, _stream()), "npvp_convt3x3s2_f16")
        tag_amax(y, y_slot)                                             # (amax_of looks at a view's base)
        out = tag_amax(y.permute(0, 3, 1, 2), y_slot)
        ctx.act, ctx.dims = act, (Fr, C_in, H, W, C_out)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(out, bwd, bwd_w_amax, zero_bias)
        return out

    @scoped
    def backward(ctx, g):
        y, bwd, bwd_w_amax, zero_bias = ctx.saved_tensors
        Fr, C_in, H, W, C_out = ctx.dims
        g = g.contiguous(memory_format=torch.channels_last)
        if ctx.act != 0:
            dz = torch.empty_like(g)
            check(lib().npvp_act_bwd(_ptr(g), _ptr(y), _ptr(dz), y.numel(), ctx.act, _stream()), "npvp_act_bwd")
            g = dz
        s = AmaxSlot.new(g.device)
        check(lib().npvp_amax(_ptr(g), Fr * 4 * H * W, C_out, C_out, _ptr(s), _stream()), "npvp_amax")
        dx = torch.empty((Fr, H, W, C_in), device=g.device, dtype=torch.float32)
        check(lib().npvp_conv3x3s2_f16(_ptr(g), _ptr(bwd), _ptr(zero_bias), None, _ptr(dx), Fr, 2 * H, 2 * W, C_out, C_in, 0, _ptr(s),
                                       _ptr(bwd_w_amax), None, None, 0, _stream()), "npvp_conv3x3s2_f16")
        return dx.permute(0, 3, 1, 2), None, None, None, None, None, None, None


def convt3x3s2_packed(x, planes, bias, act=0):
    """y = act(conv_transpose2d(x, w, stride 2, padding 1, output_padding 1) + bias[c]) of a frozen upsampling convolution on
    channels-last frames x (F, C_in, H, W) -> (F, C_out, 2H, 2W), one npvp_convt3x3s2_f16 launch (the transposed form of
    conv3x3_packed's kernel).  planes: convt3x3s2_planes of the folded weight.  The amax slot of x is its producer's or one npvp_amax
    pass (amax_of); the slot of y is attached to the result and to its NCHW view, so a following convt3x3s2_packed needs no pass.
    Differentiable w.r.t. x (act_bwd, amax, one npvp_conv3x3s2_f16).  x must be channels-last (no silent copy)."""
    _chk(x, bias, planes.w_amax, planes.bwd_w_amax, planes.zero_bias)
    if x.dim() != 4 or bias.dim() != 1:
        raise RuntimeError("convt3x3s2_packed: x must be (F, C_in, H, W) and bias (C_out,)")
    C_in, C_out = x.shape[1], bias.shape[0]
    if not convt3x3s2_takes(C_in, C_out):
        raise RuntimeError("convt3x3s2_packed: C_in and C_out must be multiples of 64")
    for p in (planes.fwd, planes.bwd):
        if p.numel() != 2 * 9 * C_in * C_out or not p.is_cuda or p.dtype != torch.float16:
            raise RuntimeError("convt3x3s2_packed: planes do not belong to a [C_in][C_out][3][3] weight of these channel counts")
    if planes.zero_bias.numel() != C_in:
        raise RuntimeError("convt3x3s2_packed: planes do not belong to a [C_in][C_out][3][3] weight of these channel counts")
    if not x.permute(0, 2, 3, 1).is_contiguous():
        raise RuntimeError("convt3x3s2_packed: x must be channels-last")
    return _ConvT3x3S2.apply(x, _c(bias), act, *planes)


# --------------------------------------------------------------------------- frozen decoder: the 7 x 7 tail (csrc/conv7x7.hip)
TAIL7X7_ACTS = (0, 2, 3)         # none, Tanh, Sigmoid


def tail7x7_takes(C_in, C_out):
    """channel counts of a ReflectionPad2d(3) -> Conv2d(C_in, C_out, 7) the route runs: a K-step of 32 inside one kernel row, the
    output channels padded to 4 inside the 32 GEMM columns"""
    return C_in > 0 and C_in % 32 == 0 and C_in <= 4096 and 1 <= C_out <= 4


Tail7x7Planes = namedtuple("Tail7x7Planes", "fwd w_amax bwd")


def tail7x7_planes(w):
    """the planes of a frozen Conv2d weight w [C_out][C_in][7][7] for tail7x7_packed: fwd (npvp_tail7x7_planes, K ordered (kh, ci),
    columns (kw, co)), the weight's amax slot, and bwd, the input gradient's planes at the scale of the same slot
    (npvp_tail7x7_dgrad_planes)"""
    _chk(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (7, 7) or not tail7x7_takes(w.shape[1], w.shape[0]):
        raise RuntimeError("tail7x7_planes: w must be [C_out][C_in][7][7] with C_in a multiple of 32 and 1 <= C_out <= 4")
    w = w.detach().contiguous()
    C_out, C_in = w.shape[:2]
    L = lib()
    halves = L.npvp_tail7x7_planes_bytes(C_in, C_out) // 2
    fwd = torch.empty(halves, dtype=torch.float16, device=w.device)
    bwd = torch.empty(halves, dtype=torch.float16, device=w.device)
    slot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(L.npvp_tail7x7_planes(_ptr(w), C_in, C_out, _ptr(fwd), _ptr(slot), _stream()), "npvp_tail7x7_planes")
    check(L.npvp_tail7x7_dgrad_planes(_ptr(w), C_in, C_out, _ptr(bwd), _ptr(slot), _stream()), "npvp_tail7x7_dgrad_planes")
    return Tail7x7Planes(fwd, slot, bwd)


class _Tail7x7(_Function):
    """y = act(conv2d(reflection_pad(x, 3), w) + bias[c]) of a frozen 7 x 7 weight with C_out <= 4: channels-last x in, contiguous
    NCHW y out.  Gradient w.r.t. x only: npvp_act_bwd through the saved OUTPUT (planar), one npvp_amax pass, one
    npvp_tail7x7_dgrad_f16 launch; dx is channels-last."""

    @staticmethod
    def forward(ctx, x, bias, act, fwd, w_amax, bwd):
        remember(ctx)
        Fr, C_in, H, W = x.shape
        C_out = bias.shape[0]
        x_slot = amax_of(x.permute(0, 2, 3, 1).reshape(Fr * H * W, C_in))            # (a view of x: finds the slot its producer attached)
        y = torch.empty((Fr, C_out, H, W), device=x.device, dtype=torch.float32)
        check(lib().npvp_tail7x7_f16(_ptr(x), _ptr(fwd), _ptr(bias), _ptr(y), Fr, H, W, C_in, C_out, act, _ptr(x_slot), _ptr(w_amax),
                                     None, 0, _stream()), "npvp_tail7x7_f16")
        ctx.act, ctx.dims = act, (Fr, C_in, H, W, C_out)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(y, bwd, w_amax)
        return y

    @scoped
    def backward(ctx, g):
        y, bwd, w_amax = ctx.saved_tensors
        Fr, C_in, H, W, C_out = ctx.dims
        n = y.numel()
        npad = (n + 3) // 4 * 4                          # npvp_amax reads float4s: a zero tail behind dz where n is no multiple of 4
        g = _c(g)
        if ctx.act != 0 or npad != n:
            dz = torch.empty(npad, device=g.device, dtype=torch.float32)
            if npad != n:
                dz[n:].zero_()
            if ctx.act != 0:
                check(lib().npvp_act_bwd(_ptr(g), _ptr(y), _ptr(dz), n, ctx.act, _stream()), "npvp_act_bwd")
            else:
                dz[:n].copy_(g.view(-1))
        else:
            dz = g
        s = AmaxSlot.new(g.device)
        check(lib().npvp_amax(_ptr(dz), 1, npad, npad, _ptr(s), _stream()), "npvp_amax")
        dx = torch.empty((Fr, H, W, C_in), device=g.device, dtype=torch.float32)
        check(lib().npvp_tail7x7_dgrad_f16(_ptr(dz), _ptr(bwd), _ptr(dx), Fr, H, W, C_in, C_out, _ptr(s), _ptr(w_amax), None, 0, _stream()),
              "npvp_tail7x7_dgrad_f16")
        return dx.permute(0, 3, 1, 2), None, None, None, None, None


def tail7x7_packed(x, planes, bias, act=0):
    """y = act(conv2d(reflection_pad2d(x, 3), w) + bias[c]) of the frozen decoder's 7 x 7 output convolution on channels-last frames
    x (F, C_in, H, W) -> contiguous NCHW (F, C_out, H, W), one npvp_tail7x7_f16 launch: the padding is index math, bias and activation
    are the epilogue.  planes: tail7x7_planes of the folded weight.  act: 0 none, 2 Tanh, 3 Sigmoid.  The amax slot of x is its
    producer's or one npvp_amax pass (amax_of).  Differentiable w.r.t. x (act_bwd, amax, one npvp_tail7x7_dgrad_f16; dx is
    channels-last).  x must be channels-last (no silent copy); H, W >= 4, as reflection by 3 needs."""
    _chk(x, bias, planes.w_amax)
    if x.dim() != 4 or bias.dim() != 1:
        raise RuntimeError("tail7x7_packed: x must be (F, C_in, H, W) and bias (C_out,)")
    C_in, C_out = x.shape[1], bias.shape[0]
    if not tail7x7_takes(C_in, C_out):
        raise RuntimeError("tail7x7_packed: C_in must be a multiple of 32 and 1 <= C_out <= 4")
    if act not in TAIL7X7_ACTS:
        raise RuntimeError("tail7x7_packed: act is 0 (none), 2 (Tanh) or 3 (Sigmoid)")
    if x.shape[2] < 4 or x.shape[3] < 4:
        raise RuntimeError("tail7x7_packed: H and W must be at least 4 (ReflectionPad2d(3))")
    for p in (planes.fwd, planes.bwd):
        if p.numel() != 2 * 7 * C_in * 32 or not p.is_cuda or p.dtype != torch.float16:
            raise RuntimeError("tail7x7_packed: planes do not belong to a [C_out][C_in][7][7] weight of this C_in")
    if not x.permute(0, 2, 3, 1).is_contiguous():
        raise RuntimeError("tail7x7_packed: x must be channels-last")
    return _Tail7x7.apply(x, _c(bias), act, *planes)


# --------------------------------------------------------------------------- frozen encoder: the 7 x 7 stem (csrc/conv7x7.hip)
STEM7X7_ACTS = (0, 1)            # none, ReLU


def stem7x7_takes(C_in, C_out):
    """channel counts of a ReflectionPad2d(3) -> Conv2d(C_in, C_out, 7) the stem kernel runs: thin K (the image's channels), C_out in
    32-column tiles"""
    return 1 <= C_in <= 4 and C_out > 0 and C_out % 32 == 0 and C_out <= 4096


def stem7x7_planes(w):
    """(planes, w_amax) of a frozen weight w [C_out][C_in][7][7] for stem7x7_packed: the scaled two-term fp16 planes npvp_stem7x7_f16
    reads, K ordered (kh, kw, ci) and zero-padded to a multiple of 32, and the weight's amax slot as a 512-float tensor"""
    _chk(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (7, 7) or not stem7x7_takes(w.shape[1], w.shape[0]):
        raise RuntimeError("stem7x7_planes: w must be [C_out][C_in][7][7] with 1 <= C_in <= 4 and C_out a multiple of 32")
    w = w.detach().contiguous()
    C_out, C_in = w.shape[:2]
    planes = torch.empty(lib().npvp_stem7x7_planes_bytes(C_in, C_out) // 2, dtype=torch.float16, device=w.device)
    slot = torch.zeros(AmaxSlot.FLOATS, device=w.device)
    check(lib().npvp_stem7x7_planes(_ptr(w), C_in, C_out, _ptr(planes), _ptr(slot), _stream()), "npvp_stem7x7_planes")
    return planes, slot


def _planar_amax(x):
    """the amax slot of planar frames x (F, C, H, W), contiguous: its producer's, or one npvp_amax pass over the memory viewed as one
    row (npvp_amax reads float4s: where the element count is no multiple of 4 - no frame size of the configs - the last 1..3 elements go
    through a second pass over a zero-padded copy of those few floats)"""
    for cand in (x, x._base):                            # as amax_of: a view is bounded by the slot of the tensor it is a view of
        tag = getattr(cand, "_npvp_amax", None) if cand is not None else None
        if tag is not None and tag[1] == cand._version:
            return tag[0]
    if x.data_ptr() % 16:
        raise RuntimeError("stem7x7_packed: x carries no amax slot and does not start at a 16-byte boundary (npvp_amax reads float4s)")
    flat = x.reshape(-1)                                 # a view: x is contiguous
    n = flat.numel()
    s, n4 = AmaxSlot.new(x.device), n - n % 4
    if n4:
        check(lib().npvp_amax(_ptr(flat), 1, n4, n4, _ptr(s), _stream()), "npvp_amax")
    if n4 != n:
        rest = torch.zeros(4, device=x.device)
        rest[:n - n4] = flat[n4:]
        check(lib().npvp_amax(_ptr(rest), 1, 4, 4, _ptr(s), _stream()), "npvp_amax")
    return s


def stem7x7_packed(x, planes, w_amax, bias, act=1, want_amax=True):
    """y = act(conv2d(reflection_pad2d(x, 3), w) + bias[c]) of the frozen encoder's 7 x 7 input convolution on PLANAR frames
    x (F, C_in, H, W) (contiguous NCHW, as the data path hands them over; with C_in = 1 that is the channels-last memory as well) ->
    channels-last (F, C_out, H, W), one npvp_stem7x7_f16 launch: the padding is index math, bias and activation are the epilogue.
    planes / w_amax: stem7x7_planes of the folded weight.  act: 0 none, 1 ReLU.  The amax slot of x is its producer's or one npvp_amax
    pass over the planar memory; want_amax attaches the slot of y to the result and to its NCHW view, so a following conv3x3s2_packed
    needs no pass.  Forward only: an input that requires grad is refused.  x in any other layout is refused (no silent copy); H, W >= 4,
    as reflection by 3 needs."""
    ts = [t for t in (x, bias) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise NotImplementedError("stem7x7_packed: forward only (the frozen encoder's input convolution); an input requires grad")
    _chk(x, w_amax, bias)
    if x.dim() != 4 or bias.dim() != 1:
        raise RuntimeError("stem7x7_packed: x must be (F, C_in, H, W) and bias (C_out,)")
    Fr, C_in, H, W = x.shape
    C_out = bias.shape[0]
    if not stem7x7_takes(C_in, C_out):
        raise RuntimeError("stem7x7_packed: 1 <= C_in <= 4 and C_out must be a multiple of 32")
    if act not in STEM7X7_ACTS:
        raise RuntimeError("stem7x7_packed: act is 0 (none) or 1 (ReLU)")
    if H < 4 or W < 4:
        raise RuntimeError("stem7x7_packed: H and W must be at least 4 (ReflectionPad2d(3))")
    if planes.numel() != 2 * ((49 * C_in + 31) // 32 * 32) * C_out or not planes.is_cuda or planes.dtype != torch.float16:
        raise RuntimeError("stem7x7_packed: planes do not belong to a [C_out][C_in][7][7] weight of these channel counts")
    if not x.is_contiguous():
        raise RuntimeError("stem7x7_packed: x must be planar (contiguous NCHW) frames")
    x_slot = _planar_amax(x)
    y = torch.empty((Fr, H, W, C_out), device=x.device, dtype=torch.float32)
    y_slot = AmaxSlot.new(x.device) if want_amax else None
    check(lib().npvp_stem7x7_f16(_ptr(x), _ptr(planes), _ptr(_c(bias)), _ptr(y), Fr, H, W, C_in, C_out, act, _ptr(x_slot), _ptr(w_amax),
                                 _ptr(y_slot), None, 0, _stream()), "npvp_stem7x7_f16")
    tag_amax(y, y_slot)                                             # (amax_of looks at a view's base)
    return tag_amax(y.permute(0, 3, 1, 2), y_slot)


# --------------------------------------------------------------------------- Stage-1 autoencoder training (csrc/ae_train.hip)
class _BnActTrain(_Function):
    """BatchNorm2d (batch statistics in training, running statistics in eval) -> act (0 none, 1 ReLU) [-> + residual] as one
    statistics pass and one apply pass forward, one sum pass and one dx pass backward (npvp_bn_*).
    group (training mode only; synchronised BatchNorm, Lightning's sync_batchnorm=True, ref/train_AutoEncoder_lightning.py:40-42):
    the statistics span the ranks of that process group - ONE all-reduce of [sum x, sum x^2, n] (double) between the statistics pass
    and the apply pass, one of [sum g', sum g' xhat] between the backward's two passes (npvp_bn_act_apply_sync / npvp_bn_bwd_sums /
    npvp_bn_act_bwd_apply).  dw / db stay this rank's own sums: the gradient all-reduce finishes them."""

    @staticmethod
    def forward(ctx, x, w, b, residual, running_mean, running_var, momentum, eps, act, train, group=None):
        remember(ctx)
        _chk(x, w, b, residual, running_mean, running_var)
        x, outer, inner, layout = _nchw_layout(x, "bn_act_train")
        C = x.shape[1]
        if w.shape != (C,) or b.shape != (C,):
            raise RuntimeError(f"bn_act_train: weight / bias must be ({C},)")
        if residual is not None:
            if residual.shape != x.shape:
                raise RuntimeError("bn_act_train: residual shape differs from x")
            residual = residual.contiguous(memory_format=_memory_format(layout))
        if not train and running_mean is None:
            raise RuntimeError("bn_act_train: eval mode needs running statistics")
        L = lib()
        y = torch.empty_like(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        group = group if train else None
        stat, count = None, 0                           # [sum x, sum x^2] in double; with a group: followed by n
        if train:
            stat = torch.empty(2 * C + (group is not None), dtype=torch.float64, device=x.device)
            ws, wsn = _ws(L.npvp_bn_workspace_bytes(C), x.device)
            check(L.npvp_bn_stats(_ptr(x), outer, inner, C, layout, _ptr(stat), _ptr(ws), wsn, _stream()), "npvp_bn_stats")
            count = outer * inner // C
        rm, rv = _ptr(running_mean), _ptr(running_var)  # (updated in training mode, read in eval mode; None: not tracked)
        if group is None:
            check(L.npvp_bn_act_apply(_ptr(x), _ptr(w), _ptr(b), _ptr(residual), _ptr(stat), count, float(eps), float(momentum or 0.0), rm, rv,
                                      outer, inner, C, layout, act, _ptr(y), _ptr(mean), _ptr(rstd), _stream()), "npvp_bn_act_apply")
        else:
            from . import dp
            import torch.distributed as dist
            stat[2 * C:].fill_(float(count))            # (a fill kernel, not a host-to-device copy)
            dp._collective(lambda: dist.all_reduce(stat, group=group))
            check(L.npvp_bn_act_apply_sync(_ptr(x), _ptr(w), _ptr(b), _ptr(residual), _ptr(stat), float(eps), float(momentum or 0.0), rm, rv,
                                           outer, inner, C, layout, act, _ptr(y), _ptr(mean), _ptr(rstd), _stream()), "npvp_bn_act_apply_sync")
        ctx.save_for_backward(x, w, b, mean, rstd, stat if group is not None else None)
        ctx.act, ctx.train, ctx.group, ctx.has_res = act, bool(train), group, residual is not None
        return y

    @scoped
    def backward(ctx, g):
        x, w, b, mean, rstd, stat = ctx.saved_tensors
        _chk(g)
        x, outer, inner, layout = _nchw_layout(x, "bn_act_train")
        g = g.contiguous(memory_format=_memory_format(layout))
        C, group = x.shape[1], ctx.group
        L = lib()
        dx = torch.empty_like(x)
        dw = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty_like(dw)
        ws, wsn = _ws(L.npvp_bn_workspace_bytes(C), x.device)
        saved, shape = (_ptr(g), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b)), (outer, inner, C, layout, ctx.act)
        if group is None:
            check(L.npvp_bn_act_bwd(*saved, *shape, int(ctx.train), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), wsn, _stream()),
                  "npvp_bn_act_bwd")
        else:
            from . import dp
            import torch.distributed as dist
            sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
            check(L.npvp_bn_bwd_sums(*saved, *shape, _ptr(sums), _ptr(dw), _ptr(db), _ptr(ws), wsn, _stream()), "npvp_bn_bwd_sums")
            dp._collective(lambda: dist.all_reduce(sums, group=group))
            check(L.npvp_bn_act_bwd_apply(*saved, _ptr(sums), stat.data_ptr() + 2 * C * 8, *shape, _ptr(dx), _stream()),
                  "npvp_bn_act_bwd_apply")
        return dx, dw, db, (g if ctx.has_res else None), None, None, None, None, None, None, None


def bn_act_train(x, w, b, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=0, train=True, residual=None, group=None):
    """act(batch_norm(x)) (+ residual) for an (N,C,H,W) fp32 tensor, contiguous (NCHW planes) or channels_last (rows); running
    statistics are updated in place in training mode (torch's momentum rule, unbiased variance).  group: a torch.distributed process
    group whose ranks share the batch statistics in training mode (synchronised BatchNorm; shards may be uneven); None, or eval
    mode: this rank's own, the launch sequence unchanged"""
    if act not in (0, 1):
        raise RuntimeError("bn_act_train: act must be 0 (none) or 1 (ReLU)")
    if train and running_mean is not None and momentum is None:
        raise RuntimeError("bn_act_train: momentum=None (cumulative average) is not supported")
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("bn_act_train: running_mean and running_var go together")
    return _BnActTrain.apply(x, w, b, residual, running_mean, running_var, momentum, eps, act, bool(train), group if train else None)


_NL_GRID = {8: 64, 16: 32, 32: 16, 64: 8}        # attention dim A -> side of the AE configs' square grid at C = 8 A; value dim = 4 A (csrc/ae_attn_dims.h)


class _PackedAttn(_Function):
    """softmax(q k^T) v (unscaled scores) from ONE projection tensor qkv [rows, ld] = [q | k | v | zero padding], rows = n0*n1*n2; the
    gradient comes back in the same layout, its pad columns zero.  <export>_fwd / <export>_bwd are the C entry points, (n0, n1, n2)
    their three leading ints:
      "npvp_nonlocal_attn" (F, H, W)       NonLocalAttenion2D at the AE configs' grids: keys / values 2x2 max-pooled in the kernels
      "npvp_nonlocal_attn_grid" (F, H, W)  the same on any H x W: floor pooling, the never-pooled last line / column of an odd grid
                                           gets dk = dv = 0 from the backward's own kernels
      "npvp_temporal_attn" (N, T, HW)      NonLocalAttenion1D (ref/models/submodules.py:229-237) over the T <= TEMPORAL_ATTN_MAX_T frames
                                           of every pixel of channels-last token rows (row = (n T + t) HW + p); one backward launch
      "npvp_temporal_attn_long" (N, T, HW) the same for any T: the keys are tiled above TEMPORAL_ATTN_MAX_T frames, at or below it the
                                           launches and the bits are npvp_temporal_attn's
    scratch: the backward hands <export>_bwd a scratch D [2][rows] after lse (every export but "npvp_temporal_attn")."""

    @staticmethod
    def forward(ctx, qkv, n0, n1, n2, A, V, export, scratch):
        remember(ctx)
        _chk(qkv)
        qkv = _c(qkv)
        ld, rows = qkv.shape[1], n0 * n1 * n2
        o = torch.empty(rows, V, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(rows, dtype=torch.float32, device=qkv.device)
        p = qkv.data_ptr()
        check(getattr(lib(), export + "_fwd")(p, ld, p + 4 * A, ld, p + 8 * A, ld, _ptr(o), V, _ptr(lse), n0, n1, n2, A, V, _stream()),
              export + "_fwd")
        ctx.save_for_backward(qkv, lse)
        ctx.dims = (n0, n1, n2, A, V, export, scratch)
        return o

    @scoped
    def backward(ctx, go):
        qkv, lse = ctx.saved_tensors
        n0, n1, n2, A, V, export, scratch = ctx.dims
        _chk(go)
        go = _c(go)
        ld = qkv.shape[1]
        dqkv = torch.empty_like(qkv)
        if ld > 2 * A + V:
            dqkv[:, 2 * A + V:].zero_()
        D = [torch.empty(2 * n0 * n1 * n2, dtype=torch.float32, device=qkv.device)] if scratch else []
        p, d = qkv.data_ptr(), dqkv.data_ptr()
        check(getattr(lib(), export + "_bwd")(p, ld, p + 4 * A, ld, p + 8 * A, ld, _ptr(go), V, _ptr(lse), *map(_ptr, D),
                                              d, ld, d + 4 * A, ld, d + 8 * A, ld, n0, n1, n2, A, V, _stream()), export + "_bwd")
        return dqkv, None, None, None, None, None, None, None


def _check_qkv(name, qkv, n0, n1, n2, A, V, temporal=False):
    """the qkv [n0*n1*n2, >= 2A+V] check of every packed op.  temporal: (n0, n1, n2) = (N, T, HW) with N, HW >= 1 (T has the op's own
    check), and the kernels read the rows as float4: a row length % 4 == 0"""
    rows, ok = ("N*T*HW", n0 >= 1 and n2 >= 1) if temporal else ("F*H*W", True)
    if not ok or qkv.dim() != 2 or qkv.shape[0] != n0 * n1 * n2 or qkv.shape[1] < 2 * A + V:
        raise RuntimeError(f"{name}: qkv must be [{rows}, >= {2 * A + V}]" + (" with N, HW >= 1" if temporal else ""))
    if temporal and qkv.shape[1] % 4:
        raise RuntimeError(f"{name}: the row length of qkv ({qkv.shape[1]}) must be a multiple of 4")


def _nl_unpacked(packed, name, q, k, v, H, W):
    """q, k, v (F, H*W, a / a / v) -> packed(q | k | v as one [F*H*W, 2a+v] tensor) as (F, H*W, v)"""
    F, P, A = q.shape
    V = v.shape[-1]
    if k.shape != q.shape or v.shape[:2] != q.shape[:2] or P != H * W:
        raise RuntimeError(f"{name}: q / k (F, H*W, a), v (F, H*W, v)")
    qkv = torch.cat([q.reshape(F * P, A), k.reshape(F * P, A), v.reshape(F * P, V)], 1)
    return packed(qkv, F, H, W, A, V).view(F, P, V)


def nonlocal_attn_dims(A, V):
    """True where the non-local attention kernels have an instantiation for (attn dim, value dim)"""
    return A in _NL_GRID and V == 4 * A


def nonlocal_attn_config_shape(A, V, H, W):
    """True where (A, V) and the H x W grid are a pair of the shipped AE configs: what nonlocal_attn_packed accepts (_NL_GRID)"""
    return nonlocal_attn_dims(A, V) and H * W == _NL_GRID[A] ** 2 and H % 2 == 0 and W & (W - 1) == 0


def nonlocal_attn_packed(qkv, F, H, W, A, V):
    """qkv [F*H*W, ld >= 2A+V] (columns q | k | v, k and v UNPOOLED) -> softmax(q pool(k)^T) pool(v)  [F*H*W, V]"""
    if not nonlocal_attn_dims(A, V):
        raise RuntimeError(f"nonlocal_attn: (attn dim, value dim) = ({A}, {V}) is not one of the AE configs' {[(a, 4 * a) for a in _NL_GRID]}")
    if not nonlocal_attn_config_shape(A, V, H, W):
        raise RuntimeError(f"nonlocal_attn: a {H}x{W} grid at C = {8 * A} is not one of the AE configs' "
                           f"({', '.join(f'{s}x{s} @ {8 * a}' for a, s in _NL_GRID.items())})")
    _check_qkv("nonlocal_attn", qkv, F, H, W, A, V)
    return _PackedAttn.apply(qkv, F, H, W, A, V, "npvp_nonlocal_attn", True)


def nonlocal_attn(q, k, v, H, W):
    """q, k, v (F, H*W, a / a / v) - k and v the projections BEFORE the 2x2 max-pool - -> (F, H*W, v)"""
    return _nl_unpacked(nonlocal_attn_packed, "nonlocal_attn", q, k, v, H, W)


def nonlocal_attn_grid_packed(qkv, F, H, W, A, V):
    """nonlocal_attn_packed on any grid H, W >= 2 (odd, rectangular, not a power of two): the keys / values are the
    floor(H/2) x floor(W/2) windows of nn.MaxPool2d((2, 2), stride=2); a config shape runs nonlocal_attn_packed's own kernels"""
    if not nonlocal_attn_dims(A, V):
        raise RuntimeError(f"nonlocal_attn_grid: (attn dim, value dim) = ({A}, {V}) is not one of {[(a, 4 * a) for a in _NL_GRID]}")
    if H < 2 or W < 2:
        raise RuntimeError(f"nonlocal_attn_grid: a {H}x{W} grid has no 2x2 window")
    _check_qkv("nonlocal_attn_grid", qkv, F, H, W, A, V)
    return _PackedAttn.apply(qkv, F, H, W, A, V, "npvp_nonlocal_attn_grid", True)


def nonlocal_attn_grid(q, k, v, H, W):
    """nonlocal_attn on any grid H, W >= 2"""
    return _nl_unpacked(nonlocal_attn_grid_packed, "nonlocal_attn_grid", q, k, v, H, W)


def nonlocal_attn_any_packed(qkv, F, H, W, A, V):
    """the model's call: nonlocal_attn_packed at the configs' own (C, grid) pairs (their exact-tile kernels), nonlocal_attn_grid_packed
    at any other grid; an (A, V) that no kernel has stays with the first, which refuses it.  Both are looked up here, at call time"""
    other_grid = nonlocal_attn_dims(A, V) and not nonlocal_attn_config_shape(A, V, H, W)
    op = nonlocal_attn_grid_packed if other_grid else nonlocal_attn_packed
    return op(qkv, F, H, W, A, V)


TEMPORAL_ATTN_MAX_T = 32        # npvp_temporal_attn_*: a pixel's T x T scores are not tiled over the keys


def temporal_attn_dims():
    """the (attn dim, value dim) pairs the temporal attention kernels have: the table of the 2-D kernels"""
    return [(a, 4 * a) for a in _NL_GRID]


def _ta_unpacked(packed, name, q, k, v, T):
    """q, k (M, T, a), v (M, T, v) -> packed(q | k | v as one clip of M pixels, row = t M + m) as (M, T, v)"""
    M, Tq, A = q.shape
    V = v.shape[-1]
    if k.shape != q.shape or v.shape[:2] != q.shape[:2] or Tq != T:
        raise RuntimeError(f"{name}: q / k (M, T, a), v (M, T, v)")
    qkv = torch.cat([q, k, v], 2).transpose(0, 1).reshape(T * M, 2 * A + V)
    return packed(qkv, 1, T, M, A, V).view(T, M, V).transpose(0, 1)


def temporal_attn_packed(qkv, N, T, HW, A, V):
    """qkv [N*T*HW, ld >= 2A+V] (columns q | k | v; row = (n T + t) HW + p, the channels-last encoder's token rows) ->
    softmax(q k^T) v over the T frames of each of the N*HW pixels  [N*T*HW, V]"""
    if not nonlocal_attn_dims(A, V):
        raise RuntimeError(f"temporal_attn: (attn dim, value dim) = ({A}, {V}) is not one of {temporal_attn_dims()}")
    if not 1 <= T <= TEMPORAL_ATTN_MAX_T:
        raise RuntimeError(f"temporal_attn: T = {T} frames per clip, 1 <= T <= {TEMPORAL_ATTN_MAX_T} (longer clips need key tiling)")
    _check_qkv("temporal_attn", qkv, N, T, HW, A, V, temporal=True)
    return _PackedAttn.apply(qkv, N, T, HW, A, V, "npvp_temporal_attn", False)


def temporal_attn(q, k, v, T):
    """q, k (M, T, a), v (M, T, v) - M sequences of T frames, as NonLocalAttenion1D sees them - -> (M, T, v).  (Packs the rows as
    one clip of M pixels; the model path hands its token rows to temporal_attn_packed without a copy.)"""
    return _ta_unpacked(temporal_attn_packed, "temporal_attn", q, k, v, T)


def temporal_attn_long_packed(qkv, N, T, HW, A, V):
    """temporal_attn_packed for any clip length T >= 1: above TEMPORAL_ATTN_MAX_T frames the kernels walk the keys in tiles; a clip
    that temporal_attn_packed accepts runs temporal_attn_packed's own kernels"""
    if not nonlocal_attn_dims(A, V):
        raise RuntimeError(f"temporal_attn_long: (attn dim, value dim) = ({A}, {V}) is not one of {temporal_attn_dims()}")
    if T < 1:
        raise RuntimeError(f"temporal_attn_long: T = {T} frames per clip, T >= 1")
    _check_qkv("temporal_attn_long", qkv, N, T, HW, A, V, temporal=True)
    return _PackedAttn.apply(qkv, N, T, HW, A, V, "npvp_temporal_attn_long", True)


def temporal_attn_long(q, k, v, T):
    """temporal_attn for any T >= 1: q, k (M, T, a), v (M, T, v) -> (M, T, v)"""
    return _ta_unpacked(temporal_attn_long_packed, "temporal_attn_long", q, k, v, T)


def temporal_attn_any_packed(qkv, N, T, HW, A, V):
    """the model's call: temporal_attn_packed up to TEMPORAL_ATTN_MAX_T frames, temporal_attn_long_packed above; both are looked up
    here, at call time"""
    op = temporal_attn_packed if T <= TEMPORAL_ATTN_MAX_T else temporal_attn_long_packed
    return op(qkv, N, T, HW, A, V)


class _ReflectPad(_Function):
    """ReflectionPad2d(P) forward, gather-form backward (npvp_reflect_pad)"""

    @staticmethod
    def forward(ctx, x, P):
        remember(ctx)
        _chk(x)
        x, _, _, layout = _nchw_layout(x, "reflect_pad")
        N, C, H, W = x.shape
        if not (1 <= P < H and P < W):
            raise RuntimeError(f"reflect_pad: padding {P} must be >= 1 and < the input's H, W ({H}, {W})")
        y = torch.empty((N, C, H + 2 * P, W + 2 * P), dtype=torch.float32, device=x.device, memory_format=_memory_format(layout))
        planes = N if layout == 0 else N * C
        check(lib().npvp_reflect_pad(_ptr(x), _ptr(y), planes, H, W, C, P, layout, 0, _stream()), "npvp_reflect_pad")
        ctx.geo = (N, C, H, W, P, layout)
        return y

    @scoped
    def backward(ctx, g):
        N, C, H, W, P, layout = ctx.geo
        _chk(g)
        g = g.contiguous(memory_format=_memory_format(layout))
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device, memory_format=_memory_format(layout))
        check(lib().npvp_reflect_pad(_ptr(g), _ptr(dx), N if layout == 0 else N * C, H, W, C, P, layout, 1, _stream()), "npvp_reflect_pad")
        return dx, None


def reflect_pad(x, P):
    return _ReflectPad.apply(x, int(P))
