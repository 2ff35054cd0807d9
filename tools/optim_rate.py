"""Times of the device Adam (tactile_gym_amd.optim.DeviceAdam; csrc/tg_optim.h) against torch's own optimiser step on the same device:
torch.nn.utils.clip_grad_norm_(params, 0.5) followed by torch.optim.Adam's default step (its multi-tensor path on the device) against
DeviceAdam.step(max_grad_norm=0.5), and the two plain steps.  Writes profiles/optim_rate.txt.

  ppo policy   the reference's PPO policy on a 1 x 128 x 128 tactile image: NatureCNN with cnn_output_dim 256, pi and vf of [256, 256],
               action_net, value_net and log_std: 21 tensors
  sac critic   the reference's SAC critic on the same image: NatureCNN with cnn_output_dim 256 and two q-nets of [256, 256] on 256 + 2
               inputs: 20 tensors (tools/sac_loss_rate.py's list)

Every candidate steps its own copy of the parameters with the same fixed gradients (torch's clip rescales its copy's gradients in place, as
it does in training; once their norm is below the bound the coefficient is 1 and the kernels are the same).  The protocol is
tools/loss_head_rate.py's, whose helpers are used: device events round `--iters` back-to-back calls and the host wall time of the same
calls, the median over `--runs` runs (at least 20), the candidates alternated run by run after `--warmup` calls each; kernel counts of one
call by torch's profiler.

    python tools/optim_rate.py [--runs 30] [--iters 50] [--warmup 20] [--out profiles/optim_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_head_rate import compare  # noqa: E402
from sac_loss_rate import critic_shapes  # noqa: E402

MAX_GRAD_NORM, LR, EPS = 0.5, 3e-4, 1e-5


def kernels(fn):
    """Device kernels of one call, by torch's profiler; None where it cannot trace the device.  loss_head_rate's count without the range
    `Optimizer.step#...` that torch's step hook records around every optimiser's step and the profiler lists on the device as well."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        n = sum(1 for name in names if not name.startswith("Optimizer.step#") and "memcpy" not in name.lower() and "memset" not in name.lower())
        return n or None
    except Exception:   # noqa: BLE001
        return None


def policy_shapes():
    cnn = [(32, 1, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (256, 9216), (256,)]
    tower = [(256, 256), (256,), (256, 256), (256,)]
    return cnn + tower + tower + [(2, 256), (2,), (1, 256), (1,), (2,)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg
    torch.manual_seed(0)
    lines = [f"# the optimiser step: us per call, median (min .. max) over {args.runs} alternated runs of {args.iters} back-to-back calls each "
             f"after {args.warmup} warm-up calls; device events | host wall; {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# torch baseline: torch.nn.utils.clip_grad_norm_(params, {MAX_GRAD_NORM}) and torch.optim.Adam(lr={LR}, eps={EPS}) with its "
             "defaults; kernels: of one call, by torch's profiler"]
    verdicts = []
    for title, shapes in (("ppo policy", policy_shapes()), ("sac critic", critic_shapes())):
        start = [0.1 * torch.randn(s, device="cuda") for s in shapes]
        grads = [0.01 * torch.randn(s, device="cuda") for s in shapes]

        def copy_of():
            params = [torch.nn.Parameter(p.clone()) for p in start]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            return params
        p_ours, p_theirs, p_ours_plain, p_theirs_plain = copy_of(), copy_of(), copy_of(), copy_of()
        ours, ours_plain = tg.DeviceAdam(p_ours, lr=LR, eps=EPS), tg.DeviceAdam(p_ours_plain, lr=LR, eps=EPS)
        theirs, theirs_plain = torch.optim.Adam(p_theirs, lr=LR, eps=EPS), torch.optim.Adam(p_theirs_plain, lr=LR, eps=EPS)

        def torch_clipped():
            torch.nn.utils.clip_grad_norm_(p_theirs, MAX_GRAD_NORM)
            theirs.step()
        # one step of each from the same state, before any timing: how far apart the two are
        ours.step(max_grad_norm=MAX_GRAD_NORM)
        torch_clipped()
        moved = max(float((a.detach() - s).abs().max()) for a, s in zip(p_theirs, start))
        err = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(p_ours, p_theirs))
        names = ("DeviceAdam.step(max_grad_norm)", "clip_grad_norm_ + Adam.step", "DeviceAdam.step()", "Adam.step")
        cands = (lambda: ours.step(max_grad_norm=MAX_GRAD_NORM), torch_clipped, ours_plain.step, theirs_plain.step)
        r = compare(list(zip(names, cands)), args)
        counts = {name: kernels(fn) for name, fn in zip(names, cands)}
        lines.append(f"{title}: {len(shapes)} tensors, {sum(p.numel() for p in start)} elements (after one step from the same state: max |ours - "
                     f"torch| {err:.2e} on steps of up to {moved:.2e})")
        for name, ((med, lo, hi), (wmed, wlo, whi)) in r.items():
            n = counts[name]
            lines.append(f"    {name:32s} {med:8.1f} us ({lo:.1f} .. {hi:.1f}) | wall {wmed:8.1f} us ({wlo:.1f} .. {whi:.1f})   "
                         f"{'kernels not counted' if n is None else f'{n} kernels'}")
        for what, a_name, t_name in (("clip + step", names[0], names[1]), ("plain step", names[2], names[3])):
            (a, alo, ahi), (t, tlo, thi) = r[a_name][0], r[t_name][0]
            wide = max((ahi - alo) / a, (thi - tlo) / t) > 0.3
            verdicts.append(f"{title}, {what}: device {a:.1f} us ({alo:.1f} .. {ahi:.1f}), torch {t:.1f} us ({tlo:.1f} .. {thi:.1f}): "
                            + ("not slower" if a <= t else "SLOWER") + " than torch"
                            + ("; the runs spread widely: compare the ranges, the medians are not a cost per call" if wide else ""))
    text = "\n".join(["# " + v for v in verdicts] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
