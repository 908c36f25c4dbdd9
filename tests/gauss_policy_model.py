"""CPU model of the continuous policy's arithmetic (csrc/ppo_train.hip: ppo_gauss_sample_kernel, ppo_head_kernel<Gaussian>), in torch ops
on whatever dtype it is given: the sampled and clamped action, the Gaussian log-probability with sigma = action_std as the STANDARD
DEVIATION, and the PPO loss head with its hand-written gradient.  tests/test_stage2_sth_host.py holds it to
torch.distributions.MultivariateNormal(scale_tril=diag(action_var)) and to float64 autograd; the GPU tests compare the kernels with it."""
import math

import torch

LOG_2PI = math.log(2 * math.pi)


def sample_action(mean, noise, sigma):
    """a = 1 - relu(1 - relu(mean + sigma * noise)): each torch op rounds once, in this order."""
    raw = mean + sigma * noise
    return 1 - torch.relu(1 - torch.relu(raw)), raw


def logprob(action, mean, sigma):
    z = (action - mean) / sigma
    return -0.5 * (z * z).sum(-1) - 2 * math.log(sigma) - LOG_2PI


def entropy(sigma):
    return 1 + LOG_2PI + 2 * math.log(sigma)


def loss_head(head, actions, sigma, old_logprobs, returns, eps_clip):
    """head (N, 3) [mean logits | value], actions (N, 2), old_logprobs / returns (N,) ->
    (logprobs, values, loss.mean(), d loss.mean() / d head) with the gradient written out by hand (autograd's rule through min / clamp)."""
    n = head.shape[0]
    mu = torch.sigmoid(head[:, :2])
    lp = logprob(actions, mu, sigma)
    v = head[:, 2]
    ratio = torch.exp(lp - old_logprobs)
    adv = returns - v
    lo, hi = 1 - eps_clip, 1 + eps_clip
    surr1, surr2 = ratio * adv, ratio.clamp(lo, hi) * adv
    loss = (-torch.minimum(surr1, surr2) - 0.01 * entropy(sigma)).mean() + 0.5 * ((v - returns) ** 2).mean()
    clamped = (ratio < lo) | (ratio > hi)
    g_ratio = torch.where(clamped, torch.where(surr1 < surr2, adv, torch.where(surr1 == surr2, 0.5 * adv, torch.zeros_like(adv))), adv)
    g_lp = -g_ratio * ratio / n
    dhead = torch.empty_like(head)
    dhead[:, :2] = g_lp[:, None] * (actions - mu) / (sigma * sigma) * mu * (1 - mu)
    dhead[:, 2] = (v - returns) / n
    return lp, v, loss, dhead
