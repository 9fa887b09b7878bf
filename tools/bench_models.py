#!/usr/bin/env python3
"""Secondary per-model step benchmarks (1 GPU, colocated split pipeline):
BERT/AGNEWS cut=2 (the reference's measured BERT cut), KWT cut=7,
MobileNetv1 cut=40, ViT cut=6 — samples/sec forward+backward+optimizer on the
native kernel path.  Evidence that the whole model zoo runs and performs."""

import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from split_learning_amd.models import build_partition  # noqa: E402
from split_learning_amd.models.lora import apply_lora  # noqa: E402
from split_learning_amd.parallel.optim import make_optimizer  # noqa: E402
from split_learning_amd.data.synthetic import SHAPES  # noqa: E402
from split_learning_amd.ops import functional as hf  # noqa: E402

LEARNING = {"learning-rate": 5e-4, "weight-decay": 0.01, "momentum": 0.5}


def bench_model(model, data, cut, batch, steps=64, warmup=16, lora=False,
                graphs=False, bert_pad_frac=None):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    s1 = build_partition(model, data, [0, cut]).to(dev).train()
    s2 = build_partition(model, data, [cut, -1]).to(dev).train()
    if lora:
        apply_lora(s1)
        apply_lora(s2, trainable_extra=(f"layer{s2.TOTAL_UNITS}.classifier",))
        s1.to(dev)
        s2.to(dev)  # LoRA adds fresh CPU parameters
    o1 = make_optimizer(model, s1.parameters(), LEARNING)
    o2 = make_optimizer(model, s2.parameters(), LEARNING)
    shape, n_labels, dtype, vocab = SHAPES[data]
    if dtype == torch.int64:
        x = torch.randint(1, vocab, (batch, *shape), device=dev)
    else:
        x = torch.randn(batch, *shape, device=dev)
    y = torch.randint(0, n_labels, (batch,), device=dev)
    if model == "BERT" and bert_pad_frac is not None:
        # padded-batch arm: the tail of every sample is pad id 0 and both
        # partitions are told the pad id (only the one that owns layer 1 sees
        # ids and masks).  0.0 pads nothing but still runs the masked path.
        n_pad = int(round(shape[0] * float(bert_pad_frac)))
        if n_pad > 0:
            x[:, shape[0] - n_pad:] = 0
        s1.mask_pad_token_id = 0
        s2.mask_pad_token_id = 0

    last = {}

    def step():
        out1 = s1(x)
        act = out1.detach().requires_grad_(True)
        loss = hf.cross_entropy(s2(act), y)
        loss.backward()
        o2.step()
        out1.backward(gradient=act.grad)
        o1.step()
        last["loss"] = loss
        return loss

    graph = None
    if graphs:
        # grads are None entering capture: AccumulateGrad steals the backward
        # kernels' outputs (no per-param add_), and the optimizer descriptor
        # is rebuilt inside capture via the pinned-memcpy path (see bench.py)
        sstream = torch.cuda.Stream()
        sstream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sstream):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(sstream)
        # keep the stolen grad buffers alive (no mid-capture free; see bench.py)
        o1.release_grads = False
        o2.release_grads = False
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()

    runner = (lambda: graph.replay()) if graph is not None else step
    for _ in range(warmup):
        runner()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {
        "model": f"{model}/{data}", "cut": cut, "batch": batch,
        "ms_per_step": round(dt / steps * 1e3, 3),
        "samples_per_sec": round(steps * batch / dt, 1),
        "lora": lora, "graphs": graphs,
        **({"bert_pad_frac": bert_pad_frac}
           if model == "BERT" and bert_pad_frac is not None else {}),
        "loss": round(float(last["loss"].detach()), 4),
    }


if __name__ == "__main__":
    # hipGraph replay is now the measured-default for EVERY model.  BERT and
    # MobileNet originally measured slower under replay, but that was before
    # the capture grad steal removed the per-parameter accumulate-add kernels
    # from the captured step (~200 for BERT+LoRA); re-measured after it:
    # BERT 1145 vs 1060 eager, MobileNet 9851 vs 7868 eager.
    # --eager disables all.  --bert-pad-frac F (opt-in) pads the tail of each
    # BERT sample and turns the attention padding mask on; --only MODEL runs
    # one arm.
    eager = "--eager" in sys.argv
    pad_frac = None
    if "--bert-pad-frac" in sys.argv:
        pad_frac = float(sys.argv[sys.argv.index("--bert-pad-frac") + 1])
    only = None
    if "--only" in sys.argv:
        only = sys.argv[sys.argv.index("--only") + 1]
    for m, d, c, b, lora, g in [("VGG16", "CIFAR10", 7, 32, False, True),
                                ("BERT", "AGNEWS", 2, 32, True, True),
                                ("KWT", "SPEECHCOMMANDS", 7, 32, False, True),
                                ("MobileNetv1", "CIFAR10", 40, 32, False, True),
                                ("ViT", "CIFAR10", 6, 32, False, True)]:
        if only is not None and m != only:
            continue
        r = bench_model(m, d, c, b, lora=lora, graphs=(g and not eager),
                        bert_pad_frac=pad_frac)
        print(json.dumps(r), flush=True)
