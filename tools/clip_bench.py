#!/usr/bin/env python3
"""What gradient-norm clipping costs per optimizer step on one GPU.

Two arms over the same parameters and gradients, alternating, timed with
device events around blocks of eager steps:

  parent  torch.nn.utils.clip_grad_norm_ on the parameters, then the fused
          optimizer step (what train_last_stage ran before the optimizer
          learnt to clip)
  new     the fused optimizer with max_grad_norm set: grad_norm_fused (two
          launches), then the fused step scaling by the coefficient

for two parameter sets: the VGG16/CIFAR10 cut=7 last stage (SGD) and the
BERT/AGNEWS cut=2 + LoRA last stage (AdamW).  Only clip + step is inside the
timed window; the gradients are fixed random tensors handed back to p.grad
before every step, as a backward would (release_grads stays on).

--launches profiles one step of each arm instead and prints its device
kernel launches by name (a run of its own: the profiler slows the host).

Prints one JSON line per parameter set.
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from split_learning_amd.models import build_partition  # noqa: E402
from split_learning_amd.models.lora import apply_lora  # noqa: E402
from split_learning_amd.parallel.optim import make_optimizer  # noqa: E402

LEARNING = {"learning-rate": 5e-4, "weight-decay": 0.01, "momentum": 0.5}
MAX_NORM = 1.0
SETS = [("VGG16", "CIFAR10", 7, False), ("BERT", "AGNEWS", 2, True)]


def _last_stage_params(model, data, cut, lora, dev):
    torch.manual_seed(0)
    s2 = build_partition(model, data, [cut, -1]).to(dev).train()
    if lora:
        apply_lora(s2, trainable_extra=(f"layer{s2.TOTAL_UNITS}.classifier",))
        s2.to(dev)  # LoRA adds fresh CPU parameters
    return [p for p in s2.parameters() if p.requires_grad]


class _Arm:
    def __init__(self, model, params, native_clip):
        # each arm steps its own copy, so neither sees the other's updates
        self.params = [p.detach().clone().requires_grad_(True) for p in params]
        self.opt = make_optimizer(model, self.params, LEARNING)
        self.native_clip = native_clip
        if native_clip:
            self.opt.max_grad_norm = MAX_NORM

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g
        if not self.native_clip:
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        self.opt.step()


def _time_block(arm, grads, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        arm.step(grads)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / inner  # us per step


def _kernel_launches(arm, grads):
    from torch.profiler import ProfilerActivity, profile
    arm.step(grads)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        arm.step(grads)
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name \
                and "Memset" not in ev.name:
            names[ev.name] = names.get(ev.name, 0) + 1
    assert names, "the profiler recorded no device kernels"
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=40, help="timed blocks per arm")
    ap.add_argument("--inner", type=int, default=50, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_bench needs a GPU"
    dev = torch.device("cuda:0")
    for model, data, cut, lora in SETS:
        params = _last_stage_params(model, data, cut, lora, dev)
        g = torch.Generator(device="cpu").manual_seed(1)
        # the restored gradients are never scaled in place by the new arm; the
        # parent arm's torch clip scales them, so each arm gets its own
        arms = {"parent": _Arm(model, params, False), "new": _Arm(model, params, True)}
        grads = {k: [torch.randn(p.shape, generator=g).to(dev) for p in params]
                 for k in arms}
        row = {"set": f"{model}/{data} cut={cut}" + (" +LoRA" if lora else ""),
               "tensors": len(params), "elements": sum(p.numel() for p in params),
               "max_norm": MAX_NORM}
        if args.launches:
            for k, arm in arms.items():
                names = _kernel_launches(arm, grads[k])
                row[f"{k}_launches"] = sum(names.values())
                row[f"{k}_kernels"] = names
        else:
            for k, arm in arms.items():
                for _ in range(args.warmup):
                    arm.step(grads[k])
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(args.blocks):
                for k, arm in arms.items():  # alternate the arms block by block
                    times[k].append(_time_block(arm, grads[k], args.inner))
            for k, ts in times.items():
                ts.sort()
                row[f"{k}_us_median"] = round(ts[len(ts) // 2], 2)
                row[f"{k}_us_min"] = round(ts[0], 2)
                row[f"{k}_us_max"] = round(ts[-1], 2)
            row["new_over_parent"] = round(row["new_us_median"] / row["parent_us_median"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
