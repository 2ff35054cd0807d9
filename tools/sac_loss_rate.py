"""Times of SAC's device losses (tactile_gym_amd.loss_head.sac_critic_loss / sac_actor_loss; csrc/tg_sac_loss.hip) and of
tactile_gym_amd.train.polyak_update against stable_baselines3's lines written with torch's own ops on the same tensors and device, forward plus
backward under torch autograd on both sides.  Writes profiles/sac_loss_rate.txt.

  critic   B = 64 and 256, n_critics = 2: from the target networks' outputs to critic_loss.backward(), gradients at both critics' outputs
  actor    B = 64 and 256, n_critics = 2: actor_loss and ent_coef_loss and their backward, gradients at log_prob, both critics' outputs and
           log_ent_coef (SB3 runs two backward passes; the fused side one, of the sum, as tg.train.sac_train does)
  polyak   a parameter list shaped like the reference's critic (NatureCNN with cnn_output_dim 256 on a 128 x 128 image, two q-nets of
           [256, 256] on 256 + 2 inputs: 20 tensors): two multi-tensor launches against SB3's two launches per tensor

The protocol is tools/loss_head_rate.py's, whose helpers are used: device events round `--iters` back-to-back calls and the host wall time of
the same calls, the median over `--runs` runs (at least 20), the candidates alternated run by run after `--warmup` calls each; kernel counts of
one call by torch's profiler.

    python tools/sac_loss_rate.py [--runs 30] [--iters 50] [--warmup 20] [--out profiles/sac_loss_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_head_rate import compare, kernels  # noqa: E402

GAMMA, TARGET_ENTROPY, TAU = 0.95, -2.0, 0.005


def torch_critic(q_cur, q_next, next_log_prob, rewards, dones, log_ent_coef):
    """SAC.train's lines as stable_baselines3 writes them, from the target networks' outputs to critic_loss."""
    import torch
    import torch.nn.functional as F
    ent_coef = torch.exp(log_ent_coef.detach())
    with torch.no_grad():
        next_q = torch.cat(q_next, dim=1)
        next_q, _ = torch.min(next_q, dim=1, keepdim=True)
        next_q = next_q - ent_coef * next_log_prob.reshape(-1, 1)
        target_q = rewards + (1 - dones) * GAMMA * next_q
    return 0.5 * sum(F.mse_loss(q, target_q) for q in q_cur)


def torch_actor(log_prob, q_pi, log_ent_coef):
    """(actor_loss, ent_coef_loss) as stable_baselines3 writes them."""
    import torch
    log_prob = log_prob.reshape(-1, 1)
    ent_coef = torch.exp(log_ent_coef.detach())
    ent_coef_loss = -(log_ent_coef * (log_prob + TARGET_ENTROPY).detach()).mean()
    min_qf_pi, _ = torch.min(torch.cat(q_pi, dim=1), dim=1, keepdim=True)
    return (ent_coef * log_prob - min_qf_pi).mean(), ent_coef_loss


def sb3_polyak(params, target_params, tau):
    import torch
    with torch.no_grad():
        for param, target_param in zip(params, target_params):
            target_param.data.mul_(1 - tau)
            torch.add(target_param.data, param.data, alpha=tau, out=target_param.data)


def critic_shapes():
    cnn = [(32, 1, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (256, 9216), (256,)]
    q_net = [(256, 258), (256,), (256, 256), (256,), (1, 256), (1,)]
    return cnn + q_net + q_net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_loss_rate.txt"))
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/sac_loss_rate.py measures on the GPU: no device found")
    import tactile_gym_amd as tg
    from tactile_gym_amd.train import polyak_update
    torch.manual_seed(0)
    lines = [f"# SAC's losses, forward + backward, and the polyak update: us per call, median (min .. max) over {args.runs} alternated runs of "
             f"{args.iters} back-to-back calls each after {args.warmup} warm-up calls; device events | host wall; "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# torch baseline: stable_baselines3's lines with torch's own ops on the same tensors, torch autograd; kernels: of one call, by "
             "torch's profiler"]
    verdicts = []

    def report(title, r, counts):
        lines.append(title)
        for name, ((med, lo, hi), (wmed, wlo, whi)) in r.items():
            n = counts[name]
            lines.append(f"    {name:28s} {med:8.1f} us ({lo:.1f} .. {hi:.1f}) | wall {wmed:8.1f} us ({wlo:.1f} .. {whi:.1f})   "
                         f"{'kernels not counted' if n is None else f'{n} kernels'}")

    def verdict(what, r, names):
        (a, alo, ahi), (t, tlo, thi) = r[names[0]][0], r[names[1]][0]
        wide = max((ahi - alo) / a, (thi - tlo) / t) > 0.3       # e.g. runs in two groups: the median then says which group held the middle run
        verdicts.append(f"{what}: fused {a:.1f} us ({alo:.1f} .. {ahi:.1f}), torch {t:.1f} us ({tlo:.1f} .. {thi:.1f}): "
                        + ("not slower" if a <= t else "SLOWER") + " than the composition"
                        + ("; the runs spread widely: compare the ranges, the medians are not a cost per call" if wide else ""))

    col = lambda B, grad=False: torch.randn(B, 1, device="cuda").requires_grad_(grad)   # noqa: E731
    for B in (64, 256):
        log_ent_coef = torch.full((1,), -0.7, device="cuda").requires_grad_()
        q_cur, q_next = [col(B, True), col(B, True)], [col(B), col(B)]
        next_log_prob, rewards = torch.randn(B, device="cuda"), col(B)
        dones = (torch.rand(B, 1, device="cuda") < 0.25).float()

        def ours():
            for t in q_cur:
                t.grad = None
            tg.sac_critic_loss(q_cur, q_next, next_log_prob, rewards, dones, GAMMA, log_ent_coef=log_ent_coef)[0].backward()

        def theirs():
            for t in q_cur:
                t.grad = None
            torch_critic(q_cur, q_next, next_log_prob, rewards, dones, log_ent_coef).backward()
        ours()
        g = q_cur[0].grad.clone()
        theirs()
        err = float((g - q_cur[0].grad).abs().max() / q_cur[0].grad.abs().max())
        names = ("tg.sac_critic_loss", "torch ops + autograd")
        r = compare(list(zip(names, (ours, theirs))), args)
        report(f"critic B = {B}, n_critics = 2 (max |ours - torch| / max |torch| of dq_cur_0 {err:.2e})", r,
               dict(zip(names, (kernels(ours), kernels(theirs)))))
        if B == 64:
            verdict("critic loss B = 64", r, names)
        log_prob, q_pi = torch.randn(B, device="cuda").requires_grad_(), [col(B, True), col(B, True)]
        leaves = [log_prob, log_ent_coef] + q_pi

        def ours():   # noqa: F811
            for t in leaves:
                t.grad = None
            actor_loss, ent_coef_loss, _ = tg.sac_actor_loss(log_prob, q_pi, log_ent_coef=log_ent_coef, target_entropy=TARGET_ENTROPY)
            (actor_loss + ent_coef_loss).backward()

        def theirs():   # noqa: F811
            for t in leaves:
                t.grad = None
            actor_loss, ent_coef_loss = torch_actor(log_prob, q_pi, log_ent_coef)
            ent_coef_loss.backward()                  # SB3: two backward passes, one per optimiser
            actor_loss.backward()
        ours()
        g = log_ent_coef.grad.clone()
        theirs()
        err = float((g - log_ent_coef.grad).abs().max() / log_ent_coef.grad.abs().max())
        names = ("tg.sac_actor_loss", "torch ops + autograd")
        r = compare(list(zip(names, (ours, theirs))), args)
        report(f"actor + ent_coef B = {B}, n_critics = 2 (|ours - torch| / |torch| of dlog_ent_coef {err:.2e})", r,
               dict(zip(names, (kernels(ours), kernels(theirs)))))
        if B == 64:
            verdict("actor and ent_coef losses B = 64", r, names)
    params = [torch.randn(s, device="cuda") for s in critic_shapes()]
    targets = [torch.randn(s, device="cuda") for s in critic_shapes()]
    names = ("tg.train.polyak_update", "SB3's per-tensor loop")
    cands = (lambda: polyak_update(params, targets, TAU), lambda: sb3_polyak(params, targets, TAU))
    r = compare(list(zip(names, cands)), args)
    report(f"polyak update, {len(params)} tensors, {sum(p.numel() for p in params)} elements (the reference's critic)", r,
           dict(zip(names, (kernels(cands[0]), kernels(cands[1])))))
    verdict("polyak update", r, names)
    text = "\n".join(["# " + v for v in verdicts] + lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
