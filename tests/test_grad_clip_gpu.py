"""Native gradient-norm clipping inside the fused optimizer step, on the GPU.

FusedSGD / FusedAdamW with max_grad_norm set launch grad_norm_fused (per-chunk
sums of squares in double, then one block that writes [norm, coef]) and hand
the coefficient to the fused step, which scales each gradient as it loads it.

Reference: float64 on the CPU, defined here: norm = sqrt(sum g^2),
coef = min(1, max_norm / (norm + 1e-6)) with torch's clamp semantics (a NaN
stays a NaN), then tests/f64_reference.py's optimizer step on g * coef.
Yardstick: torch.nn.utils.clip_grad_norm_(foreach=False) followed by
torch.optim (foreach=False) in fp32 on the GPU.  The rule is the one of
tests/test_small_kernels_f64_gpu.py:

    e_kernel <= 4 * e_torch + 4 * eps32 * max|ref64|

Tensors are carved from flat buffers with sentinel gaps (the _Flat of that
file, copied), and the sentinels of params, state and grads are checked after
every step.  Shapes are the optimizer edge set: the float4 body/tail boundary,
one element either side of the 16384-element chunk, more than one chunk, and a
parameter without a grad in the middle of the list.

Measured on an MI355X (k/t = e_kernel / e_torch, worst use of the bound):

clipped sgd     12 comparisons  k/t 1.0        adamw 0.0 step 3 m: 2.2e-10 on 1.6e-09
clipped adamw   18 comparisons  k/t 0.5 .. 1.2
norm            349.930267 against 349.9302530478613 (float64)
large grads     sgd buf 1.1e-09 on 6.7e-09, adamw v 2.6e-14 on 9.4e-14 (0.28)
"""

import copy
import math

import numpy as np
import pytest
import torch

import f64_reference as R

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
NAN, INF = float("nan"), float("inf")
SENT = 12345.0
NUMELS = [(1,), (3,), (7,), (3, 5), (16383,), (16384,), (16385,), (32773,),
          (40000,)]
NONE_AT = 4  # a parameter without grad in the middle of the list
SHAPES = NUMELS[:NONE_AT] + [(5,)] + NUMELS[NONE_AT:]
LIVE = [i for i in range(len(SHAPES)) if i != NONE_AT]
SGD_LR, ADAMW_LR = 0.1, 1e-3


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _cpu64(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def _cat(ts):
    return torch.cat([_cpu64(ts[i]).reshape(-1) for i in LIVE])


def _randn(g, scale=1.0):
    return [torch.randn(s, generator=g) * scale for s in SHAPES]


class _Flat:
    """tensors carved out of one flat buffer at offsets that are multiples of
    4 elements, 4 sentinel floats after each (and in every other gap)"""

    def __init__(self, shapes, fill):
        self.offs, off = [], 0
        for s in shapes:
            self.offs.append(off)
            off = (off + int(np.prod(s)) + 4 + 3) // 4 * 4
        self.flat = torch.full((off,), SENT, device="cuda")
        self.gap = torch.ones(off, dtype=torch.bool, device="cuda")
        self.views = []
        for s, o, f in zip(shapes, self.offs, fill):
            n = int(np.prod(s))
            v = self.flat[o:o + n].view(s)
            v.copy_(f)
            self.gap[o:o + n] = False
            self.views.append(v)

    def check_sentinels(self, what):
        assert bool((self.flat[self.gap] == SENT).all()), f"{what}: sentinel overwritten"


def _cmp(what, kernel, torch32, ref64):
    """the tolerance rule; NaN and inf placement must equal the reference's"""
    k, t, r = _cpu64(kernel), _cpu64(torch32), _cpu64(ref64)
    assert k.shape == r.shape == t.shape, f"{what}: shapes"
    nan, inf = torch.isnan(r), torch.isinf(r)
    assert torch.equal(torch.isnan(k), nan), f"{what}: NaN placement vs float64"
    assert torch.equal(torch.isnan(k), torch.isnan(t)), f"{what}: NaN placement vs torch"
    assert torch.equal(k[inf], r[inf]), f"{what}: inf placement"
    fin = ~(nan | inf)
    if not bool(fin.any()):
        return
    e_kernel = float((k[fin] - r[fin]).abs().max())
    e_torch = float((t[fin] - r[fin]).abs().max())
    bound = 4.0 * e_torch + 4.0 * EPS32 * float(r[fin].abs().max())
    print(f"CLIP | {what} | e_kernel {e_kernel:.3e} | e_torch {e_torch:.3e} | "
          f"bound {bound:.3e}")
    assert e_kernel <= bound, (
        f"{what}: e_kernel {e_kernel:.3e} > bound {bound:.3e} (e_torch {e_torch:.3e})")


def _exact(ours, theirs, what):
    """exact equality; NaN equals NaN"""
    a, b = ours.detach().cpu(), theirs.detach().cpu()
    assert a.shape == b.shape, what
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN placement"
    ok = (a == b) | torch.isnan(b)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {a.numel()} differ"


def _ref_clip(grads, max_norm):
    """float64: (norm, coef, clipped grads); max_norm None = no clipping"""
    g64 = [_cpu64(g) for g in grads]
    norm = torch.sqrt(sum((g64[i] ** 2).sum() for i in LIVE))
    if max_norm is None:
        return norm, torch.tensor(1.0, dtype=torch.float64), g64
    coef = max_norm / (norm + 1e-6)
    coef = torch.where(coef > 1.0, torch.ones_like(coef), coef)  # NaN stays
    return norm, coef, [g * coef for g in g64]


class _Rig:
    """one fused optimizer on sentinel-guarded storage, its torch twin and
    its float64 twin, stepped together.  kind "sgd": hp = (momentum, wd);
    kind "adamw": hp = wd.  max_grad_norm "absent" leaves the keyword out."""

    def __init__(self, kind, hp, max_grad_norm, seed=1, with_torch=True):
        from split_learning_amd.parallel.optim import FusedAdamW, FusedSGD
        self.kind, self.hp, self.with_torch = kind, hp, with_torch
        p0 = _randn(_gen(seed))
        zeros = [torch.zeros(s) for s in SHAPES]
        self.P = _Flat(SHAPES, p0)
        self.params = [v.requires_grad_(True) for v in self.P.views]
        kw = {} if max_grad_norm == "absent" else {"max_grad_norm": max_grad_norm}
        self.max_norm = max_grad_norm if (isinstance(max_grad_norm, float)
                                          and max_grad_norm > 0) else None
        self.tp = [p.cuda().requires_grad_(True) for p in p0]
        self.rp = [p.double() for p in p0]
        if kind == "sgd":
            m, wd = hp
            self.S = {"buf": _Flat(SHAPES, zeros)}
            self.opt = FusedSGD(self.params, lr=SGD_LR, momentum=m, weight_decay=wd, **kw)
            self.opt.bufs = self.S["buf"].views
            self.topt = torch.optim.SGD(self.tp, lr=SGD_LR, momentum=m, weight_decay=wd,
                                        foreach=False)
            self.tkeys = {"buf": "momentum_buffer"}
        else:
            self.S = {"m": _Flat(SHAPES, zeros), "v": _Flat(SHAPES, zeros)}
            self.opt = FusedAdamW(self.params, lr=ADAMW_LR, weight_decay=hp, **kw)
            self.opt.m, self.opt.v = self.S["m"].views, self.S["v"].views
            self.topt = torch.optim.AdamW(self.tp, lr=ADAMW_LR, weight_decay=hp,
                                          betas=(0.9, 0.999), eps=1e-8, foreach=False)
            self.tkeys = {"m": "exp_avg", "v": "exp_avg_sq"}
        self.opt.release_grads = False
        self.rs = {k: [z.double() for z in zeros] for k in self.S}
        self.k = 0
        self.G, self.kept = None, []
        self.ref_norm = None

    def step(self, grads, new_storage):
        """grads: CPU fp32 tensors per shape.  Returns {name: (kernel, torch,
        ref64)} over the live tensors, concatenated."""
        self.k += 1
        if new_storage or self.G is None:
            self.kept.append(self.G)  # alive, so the new one is other storage
            self.G = _Flat(SHAPES, grads)
        else:
            for v, gr in zip(self.G.views, grads):
                v.copy_(gr)
        self.ref_norm, _, clipped = _ref_clip(grads, self.max_norm)
        for i in LIVE:
            self.params[i].grad = self.G.views[i]
            self.tp[i].grad = grads[i].cuda()
            if self.kind == "sgd":
                self.rp[i], self.rs["buf"][i] = R.sgd_step(
                    self.rp[i], clipped[i], self.rs["buf"][i], SGD_LR, self.hp[0],
                    self.hp[1], self.k == 1)
            else:
                self.rp[i], self.rs["m"][i], self.rs["v"][i] = R.adamw_step(
                    self.rp[i], clipped[i], self.rs["m"][i], self.rs["v"][i], self.k,
                    ADAMW_LR, 0.9, 0.999, 1e-8, self.hp)
        self.opt.step()
        if self.with_torch:
            if self.max_norm is not None:
                torch.nn.utils.clip_grad_norm_([self.tp[i] for i in LIVE], self.max_norm,
                                               foreach=False)
            self.topt.step()
        torch.cuda.synchronize()
        for fl, name in [(self.P, "param"), (self.G, "grad")] + \
                [(fl, k) for k, fl in self.S.items()]:
            fl.check_sentinels(f"{self.kind} step {self.k} {name}")
        assert all(not bool(self.G.views[i].any()) for i in LIVE), "grads not zeroed"
        assert torch.equal(self.G.views[NONE_AT].cpu(), grads[NONE_AT]), \
            "the grad-less parameter's buffer was touched"
        out = {"p": (_cat(self.P.views), _cat(self.tp), _cat(self.rp))}
        for name, fl in self.S.items():
            if self.kind == "sgd" and self.hp[0] == 0:
                continue
            theirs = (_cat([self.topt.state[t][self.tkeys[name]] if i in LIVE else t
                            for i, t in enumerate(self.tp)])
                      if self.with_torch else _cat(self.rs[name]))
            out[name] = (_cat(fl.views), theirs, _cat(self.rs[name]))
        return out


def _three_steps(rig, seed=2, scale=1.0):
    """grad storage changes at the second step (descriptor, partial and out
    are rebuilt) and is reused at the third"""
    g = _gen(seed)
    return [rig.step(_randn(g, scale), new_storage=(k < 2)) for k in range(3)]


CONFIGS = [("sgd", (0.5, 0.0)), ("sgd", (0.9, 5e-4)), ("adamw", 0.0), ("adamw", 0.01)]


# ---------------- 1. the norm ----------------

def test_norm_within_one_ulp_and_reproducible():
    """the sum is in double, so only the final cast to float rounds; no
    atomics and a fixed order, so the same grads give the same bits"""
    grads = _randn(_gen(1))
    got = []
    for _ in range(2):
        rig = _Rig("sgd", (0.5, 0.0), 1.0, with_torch=False)
        assert rig.opt.last_grad_norm is None
        rig.step(grads, True)
        norm = rig.opt.last_grad_norm
        assert norm.is_cuda and norm.ndim == 0 and norm.dtype == torch.float32
        got.append((norm.clone(), rig.opt._desc_cache[4][1].clone()))
        ref = float(rig.ref_norm)
        print(f"CLIP | norm {float(norm):.9g} | ref64 {ref:.17g}")
        assert abs(float(norm) - ref) <= EPS32 * ref
        coef_ref = 1.0 / (ref + 1e-6)
        assert abs(float(got[-1][1][1]) - coef_ref) <= EPS32 * coef_ref
    assert torch.equal(got[0][0], got[1][0]), "norm differs between two runs"
    assert torch.equal(got[0][1], got[1][1]), "[norm, coef] differs between two runs"


# ---------------- 2. clipped update ----------------

@pytest.mark.parametrize("kind,hp", CONFIGS)
def test_clipped_update(kind, hp):
    rig = _Rig(kind, hp, 1.0)
    for k, out in enumerate(_three_steps(rig)):
        for name, (ours, theirs, ref) in out.items():
            _cmp(f"{kind} {hp} step {k + 1} {name}", ours, theirs, ref)
    assert rig.opt._desc_cache[2] == len(LIVE)


# ---------------- 3. not clipped: coefficient exactly 1 ----------------

@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_not_clipped_equals_unclipped_exactly(kind, hp):
    a, b = _Rig(kind, hp, 1e4, with_torch=False), _Rig(kind, hp, None, with_torch=False)
    for k, (oa, ob) in enumerate(zip(_three_steps(a), _three_steps(b))):
        for name in oa:
            _exact(oa[name][0], ob[name][0], f"{kind} max_norm=1e4 step {k + 1} {name}")
    assert float(a.opt._desc_cache[4][1][1]) == 1.0
    assert float(a.opt.last_grad_norm) > 100.0 and b.opt.last_grad_norm is None


# ---------------- 4. off ----------------

@pytest.mark.parametrize("off", [None, 0.0, -1.0])
@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_off_values_launch_nothing(kind, hp, off):
    a, b = _Rig(kind, hp, off, with_torch=False), _Rig(kind, hp, "absent", with_torch=False)
    for k, (oa, ob) in enumerate(zip(_three_steps(a), _three_steps(b))):
        for name in oa:
            _exact(oa[name][0], ob[name][0], f"{kind} max_grad_norm={off} step {k + 1} {name}")
    assert a.opt.last_grad_norm is None
    assert a.opt._desc_cache[4] is None, "clip buffers allocated with clipping off"


# ---------------- 5. non-finite gradients ----------------

@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_nan_grad_reaches_every_value(kind, hp):
    """one NaN gives a NaN norm and a NaN coefficient (no fmin): every updated
    value is NaN, as after torch's clip"""
    grads = _randn(_gen(3))
    grads[1][2] = NAN
    rig = _Rig(kind, hp, 1.0)
    out = rig.step(grads, True)
    assert math.isnan(float(rig.opt.last_grad_norm))
    for name, (ours, theirs, _) in out.items():
        assert bool(torch.isnan(ours).all()), f"{kind} {name}: not every value is NaN"
        assert torch.equal(torch.isnan(ours), torch.isnan(theirs)), f"{kind} {name}"
    assert torch.equal(rig.P.views[NONE_AT].cpu(), _randn(_gen(1))[NONE_AT])


@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_inf_grad_zeroes_the_rest(kind, hp):
    """one inf: norm inf, coefficient 0, so that gradient becomes NaN and the
    finite ones 0 -- everything else moves as with a zero gradient"""
    grads = _randn(_gen(3))
    grads[3][1, 2] = INF
    rig = _Rig(kind, hp, 1.0)
    out = rig.step(grads, True)
    assert float(rig.opt.last_grad_norm) == INF
    zero = _Rig(kind, hp, None, with_torch=False)
    zout = zero.step([torch.zeros(s) for s in SHAPES], True)
    for name, (ours, theirs, ref) in out.items():
        _cmp(f"{kind} inf grad {name}", ours, theirs, ref)
        nan = torch.isnan(ours)
        assert int(nan.sum()) == 1, f"{kind} {name}: {int(nan.sum())} NaN, not 1"
        _exact(ours[~nan], zout[name][0][~nan], f"{kind} inf grad {name} vs zero gradient")
    pos = sum(int(np.prod(SHAPES[i])) for i in LIVE if i < 3) + 1 * 5 + 2
    assert bool(torch.isnan(out["p"][0][pos])), "the NaN is not at the inf gradient"


@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_zero_grads_coefficient_one(kind, hp):
    zeros = [torch.zeros(s) for s in SHAPES]
    a, b = _Rig(kind, hp, 1.0, with_torch=False), _Rig(kind, hp, None, with_torch=False)
    oa, ob = a.step(zeros, True), b.step(zeros, True)
    assert float(a.opt.last_grad_norm) == 0.0
    assert float(a.opt._desc_cache[4][1][1]) == 1.0
    for name in oa:
        _exact(oa[name][0], ob[name][0], f"{kind} zero grads {name}")


# ---------------- 6. large gradients ----------------

@pytest.mark.parametrize("kind,hp", [("sgd", (0.9, 5e-4)), ("adamw", 0.01)])
def test_large_grads_do_not_overflow(kind, hp):
    """Gradients of 1e25: the true norm, about 3.5e27, fits in float.  This is
    the one deliberate difference from torch, whose fp32 sum of squares
    overflows (norm inf, coefficient 0, every gradient silently zeroed), so
    float64 alone is the reference.  Bound 4 * eps32 * max|ref64|: the scaled
    gradient carries two float roundings (the coefficient's cast and the
    product), and the value that rounds most often on top of that, AdamW's
    exp_avg_sq = (1 - beta2) * g * g, reaches 8 half-ulps = 4 eps32 at worst
    (2 x 2 from the square, the float 1 - beta2, two products, one sum)."""
    rig = _Rig(kind, hp, 1.0, with_torch=False)
    out = rig.step(_randn(_gen(4), 1e25), True)
    norm, ref = float(rig.opt.last_grad_norm), float(rig.ref_norm)
    print(f"CLIP | large norm {norm:.9g} | ref64 {ref:.17g}")
    assert math.isfinite(norm) and ref > 1e27
    assert abs(norm - ref) <= EPS32 * ref
    for name, (ours, _, r) in out.items():
        assert bool(torch.isfinite(ours).all()), f"{kind} {name}: non-finite"
        e, bound = float((ours - r).abs().max()), 4.0 * EPS32 * float(r.abs().max())
        print(f"CLIP | large {kind} {name} | e_kernel {e:.3e} | bound {bound:.3e}")
        assert e <= bound, f"{kind} large grads {name}: {e:.3e} > {bound:.3e}"
    assert float((out["p"][0] - _cat(_randn(_gen(1)))).abs().max()) > 0, "nothing moved"


# ---------------- 7. hipGraph capture ----------------

def _sgd_on(p0, b0, grads, steps_done, max_norm):
    """an eager clipped FusedSGD step from the given state"""
    from split_learning_amd.parallel.optim import FusedSGD
    params = [p.clone().requires_grad_(True) for p in p0]
    opt = FusedSGD(params, lr=SGD_LR, momentum=0.9, weight_decay=5e-4,
                   max_grad_norm=max_norm)
    opt.release_grads = False
    opt.bufs = [b.clone() for b in b0]
    opt.steps = steps_done
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    opt.step()
    return params, opt.bufs, opt.last_grad_norm


def test_capture_replays_recompute_the_coefficient():
    from split_learning_amd.parallel.optim import FusedSGD
    g = _gen(7)
    shapes = NUMELS
    max_norm = 10.0
    params = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    static_g = [torch.zeros(s, device="cuda") for s in shapes]
    for p, sg in zip(params, static_g):
        p.grad = sg
    opt = FusedSGD(params, lr=SGD_LR, momentum=0.9, weight_decay=5e-4,
                   max_grad_norm=max_norm)
    opt.release_grads = False
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            for sg in static_g:
                sg.copy_(torch.randn(sg.shape, generator=g))
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    for scale, above in ((1.0, True), (1e-3, False)):
        new = [(torch.randn(sh, generator=g) * scale).cuda() for sh in shapes]
        p0 = [p.detach().clone() for p in params]
        b0 = [b.clone() for b in opt.bufs]
        for sg, n in zip(static_g, new):
            sg.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        ep, eb, enorm = _sgd_on(p0, b0, new, 3, max_norm)
        assert (float(opt.last_grad_norm) > max_norm) == above
        assert torch.equal(opt.last_grad_norm, enorm), f"scale {scale}: norm"
        for i, (a, b) in enumerate(zip(params, ep)):
            assert torch.equal(a.detach(), b.detach()), f"scale {scale}: param {i}"
        for i, (a, b) in enumerate(zip(opt.bufs, eb)):
            assert torch.equal(a, b), f"scale {scale}: momentum buffer {i}"
        assert all(not bool(sg.any()) for sg in static_g), "grads not zeroed"


# ---------------- 8. scheduler ----------------

class _PauseWhenIdle:
    """control stub: the stage loop polls it only when no activation is
    queued, and then it answers PAUSE"""

    def recv(self, name, block=False):
        return {"action": "PAUSE"}


def test_train_last_stage_clips_natively():
    """two steps of train_last_stage against the same two steps by hand with
    torch's clip and torch.optim.SGD, and against float64 fed the hand run's
    fp32 gradients"""
    from split_learning_amd.ops import functional as hf
    from split_learning_amd.ops.modules import HipLinear
    from split_learning_amd.parallel.data_plane import LoopbackData
    from split_learning_amd.parallel.messages import ActivationMsg
    from split_learning_amd.parallel.optim import FusedSGD
    from split_learning_amd.parallel.schedulers import StageContext, train_last_stage

    clip, lr, mom = 0.05, 0.1, 0.9
    torch.manual_seed(8)
    model = torch.nn.Sequential(HipLinear(12, 16), HipLinear(16, 5)).cuda()
    twin = copy.deepcopy(model)
    g = _gen(8)
    acts = [torch.randn(4, 12, generator=g).cuda() for _ in range(2)]
    labels = [torch.randint(0, 5, (4,), generator=g).cuda() for _ in range(2)]
    plane = LoopbackData()
    for k in range(2):
        plane.send_activation(1, 0, ActivationMsg(100 + k, acts[k].clone(), labels[k], [0]))
    opt = FusedSGD(model.parameters(), lr=lr, momentum=mom)
    ctx = StageContext(client_id=1, layer_id=2, n_stages=2, cluster=0, model=model,
                       optimizer=opt, learning={}, plane=plane,
                       control=_PauseWhenIdle(), device=torch.device("cuda"),
                       clip_grad_norm=clip)
    ok, count = train_last_stage(ctx)
    assert ok and count == 8 and opt.max_grad_norm == clip
    assert float(opt.last_grad_norm) > clip, "the case must clip"

    tparams = list(twin.parameters())
    topt = torch.optim.SGD(tparams, lr=lr, momentum=mom, foreach=False)
    rp = [_cpu64(p) for p in tparams]
    rb = [torch.zeros_like(p) for p in rp]
    twin.train()
    for k in range(2):
        a = acts[k].clone().requires_grad_(True)
        topt.zero_grad()
        hf.cross_entropy(twin(a), labels[k]).backward()
        g64 = [_cpu64(p.grad) for p in tparams]
        norm = torch.sqrt(sum((x ** 2).sum() for x in g64))
        coef = min(1.0, clip / (float(norm) + 1e-6))
        for i in range(len(rp)):
            rp[i], rb[i] = R.sgd_step(rp[i], g64[i] * coef, rb[i], lr, mom, 0.0, k == 0)
        torch.nn.utils.clip_grad_norm_(tparams, clip, foreach=False)
        topt.step()
        sent = plane.recv_gradient(1, 0)
        assert sent is not None and sent.data_id == 100 + k
        if k == 0:  # same weights on both sides: the unclipped gradient, bit for bit
            assert torch.equal(sent.data, a.grad), "clipping touched the cut-layer gradient"
        else:       # weights differ in the last bits; a clipped one would be ~coef times it
            assert coef < 0.5
            torch.testing.assert_close(sent.data, a.grad, rtol=1e-3, atol=1e-6)
    flat = lambda ts: torch.cat([_cpu64(t).reshape(-1) for t in ts])
    _cmp("train_last_stage params", flat(model.parameters()), flat(tparams), flat(rp))
