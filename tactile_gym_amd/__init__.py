"""tactile_gym_amd — MI355X-native vectorised tactile-env step (drop-in for the hot path of ac-93/tactile_gym).

    import tactile_gym_amd as tg
    env = tg.make("edge_follow-v0", max_steps=200, image_size=[128, 128], env_modes={...})           # gym.Env surface
    venv = tg.make_vec("edge_follow-v0", num_envs=1024, max_steps=200, image_size=[128, 128], env_modes={...})  # VecEnv surface

The per-step arithmetic (rigid-body tick x24, tactile depth raster) runs in hand-written HIP kernels behind the C ABI
declared in include/tactile_gym_hip.h; importing the package never touches the GPU, constructing an env does and fails
loudly when the HIP library or a GPU is missing.

    K = tg.augment                                   # RAD's kornia RandomAffine translate on device tensors (imports torch)
    aug = torch.nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5))
    buf = tg.DeviceRolloutBuffer.for_env(venv, n_steps, gamma=0.95, gae_lambda=0.9)   # SB3's rollout buffer in device memory (tg.rollout; imports torch)
    for batch in buf.get(64, augment=aug): ...
    rb = tg.DeviceReplayBuffer.for_env(venv, 100_000)   # SB3's replay buffer (SAC / RAD_SAC) in device memory (tg.replay; imports torch)
    rb.start(venv.reset()); venv.step(actions); rb.add_from_env(actions); batch = rb.sample(64, augment=aug)
    vn = tg.DeviceVecNormalize(venv, gamma=0.95)        # SB3's VecNormalize on the device (tg.vecnorm; imports torch); rb.sample(64, env=vn)
    head = tg.DeviceDiagGaussian.for_env(venv)          # SB3's Gaussian sample, log-prob and clip in one launch (tg.action_head; imports torch);
    actions, env_actions, log_prob = head.sample(mean, log_std)   # tg.DeviceSquashedDiagGaussian: SAC's tanh head and its uniform warm-up
    obs, starts = tg.collect.collect_rollouts(venv, policy, buf, head, n_steps, obs, starts)   # SB3's two collection loops over the device pieces
    obs, num_timesteps = tg.collect.collect_transitions(venv, actor, rb, head, n_steps, num_timesteps, learning_starts, obs)
    loss, stats = tg.ppo_loss(mean, log_std, values, b.actions, b.old_log_prob, b.advantages, b.returns)   # PPO.train's loss and its gradients in one launch (tg.loss_head); head.rsample: SAC's
    stats = tg.train.ppo_train(policy, optimizer, buf, n_epochs, 64, 0.2, None, 0.0, 0.5, 0.5, None)      # PPO.train over the device pieces
    critic_loss, stats = tg.sac_critic_loss(q_cur, q_next, next_log_prob, b.rewards, b.dones, gamma, log_ent_coef=log_ent_coef)   # SAC.train's TD target and critic loss, one launch
    actor_loss, ent_coef_loss, stats = tg.sac_actor_loss(log_prob, q_pi, log_ent_coef=log_ent_coef, target_entropy=-A)              # its actor and entropy-coefficient losses, one launch
    critic_stats, actor_stats, n_updates = tg.train.sac_train(actor, critic, critic_target, actor_opt, critic_opt, rb, head, 1, 64, 0.95, 0.005, log_ent_coef=log_ent_coef, ent_coef_optimizer=ent_opt, target_entropy=-A)   # SAC.train over the device pieces
    heads = tg.ActorCriticHeads(features_dim, A, dict(pi=[256, 256], vf=[256, 256])); policy = lambda obs: heads(extractor(obs))   # SB3's MlpExtractor, action_net and value_net in one launch (tg.mlp; imports torch); tg.SacActorHeads, tg.ContinuousCriticHeads: SAC's
    opt = tg.DeviceAdam(params, lr=3e-4, eps=1e-5); opt.step(max_grad_norm=0.5)   # clip_grad_norm_ and Adam's step over every tensor in two launches (tg.optim; imports torch); SB3: optimizer_class=tg.DeviceAdam
    CustomCombinedExtractor(observation_space, cnn_base=tg.NatureCNN)   # SB3's NatureCNN, its first layer one launch on the uint8 images (tg.torch_layers; imports torch)
    CustomCombinedExtractor(observation_space, cnn_base=functools.partial(tg.NatureCNN, device_tail=True))   # and conv2, conv3 and the linear layer in HIP too: a row's features have one arithmetic order whatever the batch (tg.conv_relu, tg.linear_relu)
"""
from . import rl_envs  # noqa: F401  (registers the env ids)
from .registry import make, make_vec, register, registered_ids  # noqa: F401
from .vec_env import HipVecEnv  # noqa: F401  (vec_env_cls for stable_baselines3's make_vec_env)

__version__ = "0.1.0"


def __getattr__(name):
    if name in ("augment", "rollout", "replay", "vecnorm", "action_head", "collect", "torch_layers", "loss_head", "train", "mlp", "optim"):   # imported on first use: they need torch, the rest of the package does not
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "DeviceRolloutBuffer":
        import importlib
        return importlib.import_module(".rollout", __name__).DeviceRolloutBuffer
    if name == "DeviceReplayBuffer":
        import importlib
        return importlib.import_module(".replay", __name__).DeviceReplayBuffer
    if name == "DeviceVecNormalize":
        import importlib
        return importlib.import_module(".vecnorm", __name__).DeviceVecNormalize
    if name in ("DeviceDiagGaussian", "DeviceSquashedDiagGaussian"):
        import importlib
        return getattr(importlib.import_module(".action_head", __name__), name)
    if name in ("ppo_loss", "sac_critic_loss", "sac_actor_loss"):
        import importlib
        return getattr(importlib.import_module(".loss_head", __name__), name)
    if name in ("NatureCNN", "ConvStem", "conv_stem", "ConvRelu", "LinearRelu", "conv_relu", "linear_relu"):
        import importlib
        return getattr(importlib.import_module(".torch_layers", __name__), name)
    if name in ("mlp_towers", "ActorCriticHeads", "SacActorHeads", "ContinuousCriticHeads"):
        import importlib
        return getattr(importlib.import_module(".mlp", __name__), name)
    if name == "DeviceAdam":
        import importlib
        return importlib.import_module(".optim", __name__).DeviceAdam
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
