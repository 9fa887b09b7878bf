"""Gradient-norm clipping inside FusedSGD / FusedAdamW, on CPU tensors.

With max_grad_norm set the optimizers call torch.nn.utils.clip_grad_norm_ on
the live parameters before their own update loop, so every result here must
equal "clip, then the same optimizer without max_grad_norm" exactly.  The GPU
side (native norm kernels, the coefficient applied inside the fused step) is
tests/test_grad_clip_gpu.py.
"""

import copy

import pytest
import torch

from split_learning_amd.parallel.optim import FusedAdamW, FusedSGD

SHAPES = [(1,), (3, 5), (7,), (1000,)]
NONE_AT = 2  # a parameter without grad in the middle


def _make(kind, params, max_grad_norm="absent"):
    kw = {} if max_grad_norm == "absent" else {"max_grad_norm": max_grad_norm}
    if kind == "sgd":
        return FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4, **kw)
    return FusedAdamW(params, lr=1e-3, weight_decay=0.01, **kw)


def _state(opt):
    return opt.bufs if isinstance(opt, FusedSGD) else opt.m + opt.v


def _run(kind, max_grad_norm, clip_by_hand=None, steps=3, scale=1.0):
    """three steps from seeded params and grads; returns (params, state, opt)"""
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]
    opt = _make(kind, params, max_grad_norm)
    for _ in range(steps):
        for i, p in enumerate(params):
            if i != NONE_AT:
                p.grad = torch.randn(p.shape, generator=g) * scale
        if clip_by_hand is not None:
            torch.nn.utils.clip_grad_norm_(
                [p for p in params if p.grad is not None], clip_by_hand)
        opt.step()
    return [p.detach() for p in params], _state(opt), opt


@pytest.mark.parametrize("max_norm", [1.0, 1e4])  # ~32 is the norm: clips / does not
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipped_step_equals_clip_then_step(kind, max_norm):
    p, s, opt = _run(kind, max_norm)
    rp, rs, _ = _run(kind, "absent", clip_by_hand=max_norm)
    for a, b in zip(p + s, rp + rs):
        assert torch.equal(a, b)
    assert opt.last_grad_norm is not None and opt.last_grad_norm.ndim == 0
    if max_norm == 1.0:  # it did clip: the unclipped run differs
        up, _, _ = _run(kind, None)
        assert not torch.equal(p[0], up[0])


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_last_grad_norm_is_the_pre_clip_norm(kind):
    g = torch.Generator().manual_seed(6)
    params = [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]
    grads = [torch.randn(s, generator=g) for s in SHAPES]
    opt = _make(kind, params, 0.5)
    assert opt.max_grad_norm == 0.5 and opt.last_grad_norm is None
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    opt.step()
    want = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads))
    assert abs(float(opt.last_grad_norm) - float(want)) <= 1e-5 * float(want)


@pytest.mark.parametrize("off", [None, 0.0, -1.0])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_off_values_are_ignored(kind, off):
    p, s, opt = _run(kind, off)
    rp, rs, _ = _run(kind, "absent")
    for a, b in zip(p + s, rp + rs):
        assert torch.equal(a, b)
    assert opt.last_grad_norm is None


def test_attribute_switches_clipping_on_and_off():
    """max_grad_norm is a plain attribute: the scheduler sets it after
    construction"""
    p, _, _ = _run("sgd", 1.0, steps=1)
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]
    opt = _make("sgd", params)
    opt.max_grad_norm = 1.0
    for i, q in enumerate(params):
        if i != NONE_AT:
            q.grad = torch.randn(q.shape, generator=g)
    opt.step()
    for a, b in zip(p, params):
        assert torch.equal(a, b.detach())


class _PauseWhenIdle:
    """control stub: the stage loop polls it only when no activation is
    queued, and then it answers PAUSE"""

    def recv(self, name, block=False):
        return {"action": "PAUSE"}


def _two_layer(seed):
    from split_learning_amd.ops.modules import HipLinear
    torch.manual_seed(seed)
    return torch.nn.Sequential(HipLinear(12, 16), HipLinear(16, 5))


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_train_last_stage_clips_through_the_optimizer(kind):
    """train_last_stage with clip_grad_norm set: the params of the sequence it
    ran before (backward, clip_grad_norm_, step), exactly; the cut-layer
    gradients sent back are those of the unclipped backward"""
    from split_learning_amd.parallel.data_plane import LoopbackData
    from split_learning_amd.parallel.messages import ActivationMsg
    from split_learning_amd.parallel.schedulers import StageContext, train_last_stage

    clip = 0.05
    model = _two_layer(3)
    ref = copy.deepcopy(model)
    g = torch.Generator().manual_seed(4)
    acts = [torch.randn(4, 12, generator=g) for _ in range(2)]
    labels = [torch.randint(0, 5, (4,), generator=g) for _ in range(2)]

    plane = LoopbackData()
    for k in range(2):
        plane.send_activation(1, 0, ActivationMsg(100 + k, acts[k].clone(), labels[k], [0]))
    opt = _make(kind, model.parameters())
    logged = []
    ctx = StageContext(client_id=1, layer_id=2, n_stages=2, cluster=0, model=model,
                       optimizer=opt, learning={}, plane=plane,
                       control=_PauseWhenIdle(), device=torch.device("cpu"),
                       clip_grad_norm=clip, log_grad_norm=logged.append)
    ok, count = train_last_stage(ctx)
    assert ok and count == 8
    assert opt.max_grad_norm == clip
    assert ctx.pause_msg == {"action": "PAUSE"}

    ropt = _make(kind, ref.parameters())
    ref.train()
    for k in range(2):
        a = acts[k].clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(ref(a), labels[k])
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(list(ref.parameters()), clip)
        assert float(norm) > clip, "the case must clip"
        ropt.step()
        sent = plane.recv_gradient(1, 0)
        assert sent is not None and sent.data_id == 100 + k
        assert torch.equal(sent.data, a.grad), "clipping touched the cut-layer gradient"
        assert torch.equal(logged[k], norm)
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_train_last_stage_refuses_an_optimizer_that_cannot_clip():
    """clip-grad-norm with an optimizer that has no max_grad_norm is an error,
    never a step that silently goes unclipped"""
    from split_learning_amd.parallel.data_plane import LoopbackData
    from split_learning_amd.parallel.schedulers import StageContext, train_last_stage

    model = _two_layer(3)
    ctx = StageContext(client_id=1, layer_id=2, n_stages=2, cluster=0, model=model,
                       optimizer=torch.optim.SGD(model.parameters(), lr=0.1),
                       learning={}, plane=LoopbackData(), control=_PauseWhenIdle(),
                       device=torch.device("cpu"), clip_grad_norm=1.0)
    with pytest.raises(TypeError, match="clip-grad-norm"):
        train_last_stage(ctx)
    ctx.clip_grad_norm = None  # without clipping any optimizer will do
    assert train_last_stage(ctx) == (True, 0)


def test_train_last_stage_without_clip_leaves_the_optimizer_off():
    from split_learning_amd.parallel.data_plane import LoopbackData
    from split_learning_amd.parallel.schedulers import StageContext, train_last_stage

    model = _two_layer(3)
    opt = _make("sgd", model.parameters(), 1.0)
    ctx = StageContext(client_id=1, layer_id=2, n_stages=2, cluster=0, model=model,
                       optimizer=opt, learning={}, plane=LoopbackData(),
                       control=_PauseWhenIdle(), device=torch.device("cpu"),
                       clip_grad_norm=None)
    train_last_stage(ctx)
    assert opt.max_grad_norm is None
