"""Stage-2 training of the Something-Something tree without a device: the CPU model of the continuous policy's arithmetic against
torch.distributions and float64 autograd, the G19 fixture's coverage conditions, the new exports and workspace queries, the misuse
raises and the optimizer of PPO_Continuous."""
import os
import re
import types

import numpy as np
import pytest
import torch

from adafocus_amd import _lib, train
from adafocus_amd.ppo_continuous import PPO_Continuous, ActorCritic, Memory
from tests import gauss_policy_model as M
from tests.test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_sth_stage2.npz")
NEW = ("adaf_ppo_gauss_sample_f32", "adaf_ppo_gauss_head_f32", "adaf_bn_train_workspace_bytes", "adaf_bn_train_forward_f32",
       "adaf_bn_train_backward_f32", "adaf_ppo_encoder_bn_backward_workspace_bytes", "adaf_ppo_encoder_bn_backward_f32")
CASES = ("bn_vd1", "bn_vd2", "nobn_vd2", "clip")


def _mvn(mean, sigma):
    """The reference's distribution (ppo_continuous.py:96-97): diag(action_var) handed over as scale_tril, action_var = full(action_std)."""
    action_var = torch.full((2,), sigma, dtype=mean.dtype)
    return torch.distributions.MultivariateNormal(mean, scale_tril=torch.diag(action_var))


# ---- the CPU model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 0.25, 0.5])
def test_model_logprob_takes_action_std_as_the_standard_deviation(sigma):
    g = torch.Generator().manual_seed(5)
    mean = torch.rand(64, 2, generator=g, dtype=torch.float64)
    action = torch.rand(64, 2, generator=g, dtype=torch.float64)
    dist = _mvn(mean, sigma)
    assert (M.logprob(action, mean, sigma) - dist.log_prob(action)).abs().max() < 1e-12
    assert (dist.entropy() - M.entropy(sigma)).abs().max() < 1e-12
    # a variance (sigma^2 as the scale) would be a different density: the model is not that one
    wrong = torch.distributions.MultivariateNormal(mean, covariance_matrix=torch.diag(torch.full((2,), sigma, dtype=torch.float64)))
    assert (M.logprob(action, mean, sigma) - wrong.log_prob(action)).abs().min() > 1e-3


def test_model_sample_is_the_torch_expression_bit_for_bit():
    """mean + scale_tril @ z, relu, 1 - relu(1 - .) in fp32 as the reference writes it (ppo_continuous.py:98-101), with the normals the
    distribution itself drew: equal bits, clamps at both ends and interior values present."""
    sigma = 0.5
    torch.manual_seed(11)
    mean = torch.rand(4096, 2)
    dist = _mvn(mean, sigma)
    torch.manual_seed(12)
    raw_ref = dist.sample()
    torch.manual_seed(12)
    z = torch.randn(4096, 2)                 # (MultivariateNormal.sample draws standard normals of the mean's shape)
    ref = 1 - torch.nn.functional.relu(1 - torch.nn.functional.relu(raw_ref))
    got, raw = M.sample_action(mean, z, sigma)
    assert torch.equal(raw, raw_ref) and torch.equal(got, ref)
    assert (got == 0).any() and (got == 1).any() and ((got > 0) & (got < 1)).any()
    # the order matters in the last bit: 1 - (1 - x) is not x
    inside = (raw > 0) & (raw < 1)
    assert (got[inside] != raw[inside]).any()


@pytest.mark.parametrize("same", [True, False])
def test_model_loss_head_gradient_is_autograd_s(same):
    """The hand-written d loss.mean() / d head of the model against float64 autograd of the reference's expression
    (ppo_continuous.py:182-193), with ratios of one (policy_old = policy) and on both sides of the clip range."""
    n, sigma, eps = 48, 0.25, 0.2
    g = torch.Generator().manual_seed(3)
    head = torch.randn(n, 3, generator=g, dtype=torch.float64).requires_grad_()
    actions = torch.rand(n, 2, generator=g, dtype=torch.float64).round(decimals=1)      # some coordinates exactly 0 and 1
    returns = torch.randn(n, generator=g, dtype=torch.float64)
    dist = _mvn(torch.sigmoid(head[:, :2]), sigma)
    lp = dist.log_prob(actions)
    old = lp.detach().clone() if same else lp.detach() + 0.5 * torch.randn(n, generator=g, dtype=torch.float64)
    ratios = torch.exp(lp - old)
    adv = returns - head[:, 2].detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - eps, 1 + eps) * adv) + 0.5 * torch.nn.functional.mse_loss(head[:, 2], returns)
            - 0.01 * dist.entropy()).mean()
    loss.backward()
    lp_m, v_m, loss_m, dhead = M.loss_head(head.detach(), actions, sigma, old, returns, eps)
    if not same:
        r = ratios.detach()
        assert (r < 1 - eps).any() and (r > 1 + eps).any()
    assert (lp_m - lp.detach()).abs().max() < 1e-12 and abs(loss_m.item() - loss.item()) < 1e-12
    assert (dhead - head.grad).abs().max() < 1e-12 * max(1.0, head.grad.abs().max().item())


# ---- G19 -----------------------------------------------------------------------------------------------------------------------------------
def test_g19_coverage_conditions():
    g = np.load(GOLDEN)
    c, hw, h = (int(v) for v in g["dims"])
    assert (c, hw, h) == (1280, 7, 1024)
    sample_floor, ratio_floor, surr_floor = (float(v) for v in g["floors"])
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_act_stage2.npz"))
    expect = {"bn_vd1": (1, 1, 2), "bn_vd2": (1, 2, 1), "nobn_vd2": (0, 2, 1), "clip": (1, 2, 1)}
    for tag in CASES:
        with_bn, t, tg, b, k, seed_old, seed_t = (int(v) for v in g["%s_case" % tag])
        assert (with_bn, t, tg) == expect[tag] and b <= 8
        sigma = float(g["%s_action_std" % tag][0])
        mean, raw, act = (g["%s_rollout_%s" % (tag, k_)] for k_ in ("mean", "sample", "action"))
        assert mean.shape == raw.shape == act.shape == (t, b, 2) and g["%s_rollout_hidden" % tag].shape == (t, b, h)
        # the clamp: one coordinate at 0, one at 1, one interior; every raw sample clear of both edges
        assert (act == 0).any() and (act == 1).any() and ((act > 0) & (act < 1)).any()
        assert min(np.abs(raw).min(), np.abs(raw - 1).min()) >= sample_floor
        want, _ = M.sample_action(torch.from_numpy(raw), torch.zeros(t, b, 2), sigma)
        assert np.array_equal(want.numpy(), act)
        lp = M.logprob(torch.from_numpy(act).double(), torch.from_numpy(mean).double(), sigma).numpy()
        assert np.abs(lp - g["%s_rollout_logprob" % tag]).max() < 1e-5
        ret = g["%s_returns" % tag].astype(np.float64)
        assert abs(ret.mean()) < 1e-5 and abs(ret.std(ddof=1) - 1) < 1e-3
        assert np.abs(g["%s_entropy" % tag] - M.entropy(sigma)).max() < 1e-6
        if with_bn:
            assert g["%s_rollout_old_state_encoder.1.num_batches_tracked" % tag].tolist() == list(range(1, t + 1))
            assert int(g["%s_new_state_encoder.5.num_batches_tracked" % tag]) == k
        if t == 1:
            assert not g["%s_u@gru.weight_hh_l0" % tag].any()      # one step from the zero state
    assert int(g["clip_case"][4]) == 2 and int(g["clip_case"][5]) != int(g["seeds"][0])
    eps = float(g["eps_clip"][0])
    ratio = np.exp(g["clip_logprobs"].astype(np.float64) - g["clip_rollout_logprob"])
    adv = g["clip_returns"].reshape(ratio.shape).astype(np.float64) - g["clip_values"]
    lo, hi = 1 - eps, 1 + eps
    classes = [((ratio < lo) & (adv > 0)).sum(), ((ratio < lo) & (adv < 0)).sum(), ((ratio > hi) & (adv > 0)).sum(),
               ((ratio > hi) & (adv < 0)).sum()]
    assert min(classes) >= 1 and list(g["clip_classes"]) == [int(v) for v in classes]
    assert min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min()) >= ratio_floor
    assert float(g["clip_margins"][0]) >= ratio_floor and float(g["clip_margins"][1]) >= surr_floor


# ---- exports and workspace queries -----------------------------------------------------------------------------------------------------------
def test_new_exports_declared_everywhere():
    _ensure_built()
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(_lib.load_library(), name)


def test_workspace_queries_without_a_device():
    _ensure_built()
    lib = _lib.load_library()
    assert lib.adaf_bn_train_workspace_bytes(3136, 64) == 2 * 32 * 64 * 8          # two double sums x 32 row slices per column
    for bad in ((0, 64), (8, 0), (-1, 64)):
        assert lib.adaf_bn_train_workspace_bytes(*bad) == 0
    # 64 conv outputs: one [64, C] partial per pixel slice; 256 CUs / 80 chunks of 128 channels = 3 slices at the shipped shape
    npix, c = 64 * 49, 10240
    assert lib.adaf_ppo_wenc_grad_workspace_bytes(npix, c, 64) == max(3 * 64 * c, npix * 64) * 4
    t, b, hw, cmid, h = 1, 64, 49, 64, 1024
    rows, mid = t * b, hw * cmid
    plain = rows * h + rows * mid + h * mid + 32 * h + 3 * 64 * c
    assert lib.adaf_ppo_encoder_bn_backward_workspace_bytes(t, b, hw, c, cmid, h, 0) == plain * 4
    assert lib.adaf_ppo_encoder_bn_backward_workspace_bytes(t, b, hw, c, cmid, h, 1) == (plain + rows * h + rows * mid + 2 * 2 * 32 * h) * 4
    # without BatchNorm and with 32 outputs it is the discrete policy's layout
    assert lib.adaf_ppo_encoder_bn_backward_workspace_bytes(16, 64, 49, 1280, 32, 1024, 0) == \
        lib.adaf_ppo_encoder_backward_workspace_bytes(16, 64, 49, 1280, 32, 1024)
    for i in range(6):
        ext = [t, b, hw, c, cmid, h]
        ext[i] = 0
        assert lib.adaf_ppo_encoder_bn_backward_workspace_bytes(*ext, 1) == 0


def test_null_handle_is_refused_without_a_device():
    _ensure_built()
    lib = _lib.load_library()
    assert lib.adaf_ppo_gauss_sample_f32(None, None, None, 1, 0.1, None, None, None) == -1
    assert lib.adaf_ppo_gauss_head_f32(None, None, 1, 1, 1, None, 0.1, None, None, 0.2, *([None] * 8), 0, None) == -1
    assert lib.adaf_bn_train_forward_f32(None, None, 2, 64, None, None, 1e-5, 0.1, None, None, 1, None, None, None, None, 0, None) == -1
    assert lib.adaf_bn_train_backward_f32(None, None, None, None, 2, 64, *([None] * 7), 0, None) == -1
    assert lib.adaf_ppo_encoder_bn_backward_f32(*([None] * 5), 1, 2, 49, 1280, 64, 1024, *([None] * 17), 0, None) == -1


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
def _ppo(with_bn=True):
    return PPO_Continuous(256, 256 * 9, 32, True, lr=0.001, betas=(0.8, 0.99), gamma=0.6, K_epochs=3, eps_clip=0.1, action_std=0.25,
                          with_bn=with_bn)


def test_ppo_continuous_holds_an_optimizer_over_the_policy():
    ppo = _ppo()
    assert not isinstance(ppo, torch.nn.Module)
    assert (ppo.lr, ppo.betas, ppo.gamma, ppo.eps_clip, ppo.K_epochs) == (0.001, (0.8, 0.99), 0.6, 0.1, 3) and ppo.last_loss is None
    assert isinstance(ppo.optimizer, torch.optim.Adam) and len(ppo.optimizer.param_groups) == 1
    assert [id(p) for p in ppo.optimizer.param_groups[0]["params"]] == [id(p) for p in ppo.policy.parameters()]
    assert ppo.optimizer.param_groups[0]["lr"] == 0.001 and tuple(ppo.optimizer.param_groups[0]["betas"]) == (0.8, 0.99)
    # action_var is a plain attribute holding action_std itself: the state-dict keys are the reference's
    assert not any("action" in k for k in ppo.policy.state_dict())
    assert torch.equal(ppo.policy.action_var, torch.full((2,), 0.25)) and ppo.policy.action_std == 0.25
    for (k, v), (k2, v2) in zip(ppo.policy.state_dict().items(), ppo.policy_old.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)


@pytest.mark.parametrize("with_bn", [True, False])
def test_training_paths_need_the_policy_in_train_mode(with_bn):
    ppo = _ppo(with_bn)
    pol = ppo.policy_old.eval()
    state = torch.zeros(2, 256, 3, 3)
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        pol.act(state, Memory(), restart_batch=True, training=True)
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        pol.act_nhwc(torch.zeros(2, 3, 3, 256), 2, 1, Memory(), restart_batch=True, training=True)
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        pol.evaluate(torch.zeros(1, 2, 256, 3, 3), torch.zeros(1, 2, 2))
    ppo.policy.eval()
    mem = types.SimpleNamespace(rewards=[torch.zeros(1, 2)], states=[state], actions=[torch.zeros(2, 2)], logprobs=[torch.zeros(2)])
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        ppo.update(mem)


def test_one_row_with_batchnorm_is_a_value_error():
    ppo = _ppo(True)
    ppo.policy.train()
    ppo.policy_old.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ppo.policy_old.act(torch.zeros(1, 256, 3, 3), Memory(), restart_batch=True, training=True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ppo.policy.evaluate(torch.zeros(1, 1, 256, 3, 3), torch.zeros(1, 1, 2))


def test_linear_encoder_and_discrete_training_stay_out():
    pol = ActorCritic(64, 64 * 4, hidden_state_dim=32, policy_conv=False).train()
    with pytest.raises(NotImplementedError, match="policy_conv"):
        pol.act(torch.zeros(2, 64, 2, 2), Memory(), restart_batch=True, training=True)
    with pytest.raises(NotImplementedError, match="policy_conv=False"):
        pol.evaluate(torch.zeros(1, 2, 64, 2, 2), torch.zeros(1, 2, 2))
    assert "train_stage2_batch_sth" in train.__all__
