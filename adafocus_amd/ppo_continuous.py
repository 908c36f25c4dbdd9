"""Continuous patch-location policy (STH/models/ppo_continuous.py): encoder -> GRU step -> Linear(2) + Sigmoid, the producer of the (y, x)
fractions the HIP gather consumes, on the conv engine + the GRU kernel; the hidden state is carried across
``video_div`` steps in ``memory.hidden`` like the reference does.

Inference (``training=False``): the action is the mean; BatchNorm is folded from the running statistics (the reference's eval branch
still draws ``dist.sample()`` and discards it, ppo_continuous.py:98,107 -- it only advances the global RNG).

Stage-2 training (the module in train mode, ``GFV.policy_train_mode()``): ``act(training=True)`` samples
``1 - relu(1 - relu(mu + sigma z))`` from caller-drawn normals and stores state, action and log-probability; ``evaluate`` and
``PPO_Continuous.update`` are the training core of ``policy_train.py``, shared with the discrete policy, with the Gaussian head (the
policy forward over a stored roll-out through ``PolicyEvaluateFn``; returns kernel -> K_epochs x {forward, loss head, backward, Adam
step}).  BatchNorm
uses batch statistics on these paths (a roll-out step over B rows, evaluate over T*B rows) and updates the running ones.  ``action_std``
is the standard deviation itself: the reference hands ``diag(action_var)`` to MultivariateNormal as ``scale_tril``."""
import torch
from torch import nn

from . import hip_ops
from .policy_train import PolicyEvaluateFn, PolicyTrainMixin, ppo_update  # noqa: F401  (PolicyEvaluateFn: the name it had here)
from .ppo import Memory  # noqa: F401  (same class in both reference files)

__all__ = ["ActorCritic", "PPO_Continuous", "Memory"]


class ActorCritic(PolicyTrainMixin, nn.Module):
    """The training core is policy_train.PolicyTrainMixin's; this class supplies the Gaussian distribution N(mu, action_std^2 I) over (y, x)
    (constant entropy, fp32 actions (T, B, 2)), the train-mode requirement of its BatchNorm and the inference / roll-out surfaces."""
    entropy_has_grad = False
    needs_train_mode = True

    def __init__(self, feature_dim, state_dim, hidden_state_dim=1024, policy_conv=True, action_std=0.1, with_bn=False):
        super().__init__()
        if policy_conv:
            flat = int(state_dim * 64 / feature_dim)
            if with_bn:
                self.state_encoder = nn.Sequential(nn.Conv2d(feature_dim, 64, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(),
                                                   nn.Flatten(), nn.Linear(flat, hidden_state_dim),
                                                   nn.BatchNorm1d(hidden_state_dim), nn.ReLU())
            else:
                self.state_encoder = nn.Sequential(nn.Conv2d(feature_dim, 64, 1, bias=False), nn.ReLU(), nn.Flatten(),
                                                   nn.Linear(flat, hidden_state_dim), nn.ReLU())
        else:
            self.state_encoder = nn.Sequential(nn.Linear(state_dim, 2048), nn.ReLU(), nn.Linear(2048, hidden_state_dim),
                                               nn.ReLU())
        self.gru = nn.GRU(hidden_state_dim, hidden_state_dim, batch_first=False)
        self.actor = nn.Sequential(nn.Linear(hidden_state_dim, 2), nn.Sigmoid())
        self.critic = nn.Sequential(nn.Linear(hidden_state_dim, 1))
        self.hidden_state_dim, self.policy_conv, self.feature_dim = hidden_state_dim, policy_conv, feature_dim
        self.action_std = float(action_std)
        # (ppo_continuous.py:68; a plain attribute, not a buffer: the state-dict keys are the reference's)
        self.action_var = torch.full((2,), action_std)
        self.frame_channels = None       # channels of ONE glancer frame (set by the Focuser); feature_dim = Tg * that

    @torch.no_grad()
    def act_nhwc(self, featmap_nhwc, b, tg, memory=None, restart_batch=True, training=False, noise=None):
        """Clip-level action from the HIP glancer's map (B*Tg, h, w, C): the 1x1 conv over the
        channel-concatenated state (B, Tg*C, h, w) is a (Tg x 1) convolution over the (Tg, h*w) grid of
        the pixel-major map -- no concatenated tensor is built.  `memory.hidden` carries the GRU state
        across the video_div steps exactly as act() does (reset when restart_batch).
        training=True: the sampled action of stage-2 training (see _act_train)."""
        if not self.policy_conv:
            raise NotImplementedError("adafocus_amd policy: policy_conv=True (the shipped configs) only")
        if training:
            return self._act_train(featmap_nhwc, b, tg, memory, restart_batch, noise, None)
        n, hh, ww, ch = featmap_nhwc.shape
        hw = hh * ww
        enc = self.state_encoder
        with_bn = isinstance(enc[1], nn.BatchNorm2d)
        conv, lin = enc[0], enc[4 if with_bn else 3]
        cmid = conv.weight.shape[0]
        w_enc = conv.weight.detach().view(cmid, tg, 1, ch).contiguous()
        w_lin = lin.weight.detach().view(-1, cmid, hw).permute(0, 2, 1).reshape(lin.weight.shape[0], hw * cmid).contiguous()
        sc1 = bi1 = sc2 = None
        bi2 = lin.bias.detach()
        if with_bn:
            sc1, bi1 = hip_ops.fold_bn(enc[1].weight.detach(), enc[1].bias.detach(), enc[1].running_mean, enc[1].running_var)
            sc2, t2 = hip_ops.fold_bn(enc[5].weight.detach(), enc[5].bias.detach(), enc[5].running_mean, enc[5].running_var)
            bi2 = lin.bias.detach() * sc2 + t2        # BN1d(Wx + b) = (Wx) * s + (b * s + t)
        x = featmap_nhwc.view(b, tg, hw, ch)                                   # "image" of Tg rows x hw columns
        e = hip_ops.conv2d_bn_act(x, w_enc, sc1, bi1, act=hip_ops.ACT_RELU)    # (b, 1, hw, cmid)
        e = hip_ops.conv2d_bn_act(e.view(b, 1, 1, hw * cmid), w_lin.view(-1, 1, 1, hw * cmid), sc2, bi2, act=hip_ops.ACT_RELU)
        g = self.gru
        h0 = None
        if memory is not None:
            if restart_batch:      # ppo_continuous.py:79-81: the list restarts with the zero state (k + 1 entries after k steps)
                del memory.hidden[:]
                memory.hidden.append(torch.zeros(1, b, self.hidden_state_dim, device=featmap_nhwc.device))
            if memory.hidden:
                h0 = memory.hidden[-1].view(b, -1)
        hs = hip_ops.gru_seq_forward(e.view(b, 1, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(),
                                     g.bias_ih_l0.detach(), g.bias_hh_l0.detach(), h0=h0)
        if memory is not None:
            memory.hidden.append(hs.view(1, b, -1))
        a = self.actor[0]
        return hip_ops.linear(hs.view(b, -1), a.weight.detach(), a.bias.detach(), act=hip_ops.ACT_SIGMOID)

    @torch.no_grad()
    def act(self, state_ini, memory, restart_batch=False, training=False, noise=None):
        """Reference signature (ppo_continuous.py:78-109): state_ini (B, Tg*C, h, w), the glancer maps of one video_div
        segment concatenated on the channel axis.  Re-laid out pixel-major (glue) and run on the engine.  training=True: the sampled
        action; `state_ini` itself goes to memory.states."""
        b, tc, hh, ww = state_ini.shape
        ch = self.frame_channels or (1280 if tc % 1280 == 0 else tc)    # channels per glancer frame (feature_map_channels)
        tg = tc // ch
        nhwc = state_ini.view(b, tg, ch, hh, ww).permute(0, 1, 3, 4, 2).contiguous().view(b * tg, hh, ww, ch)
        if training:
            if not self.policy_conv:
                raise NotImplementedError("adafocus_amd policy: policy_conv=True (the shipped configs) only")
            return self._act_train(nhwc, b, tg, memory, restart_batch, noise, state_ini)
        return self.act_nhwc(nhwc, b, tg, memory, restart_batch)

    # ---- stage-2 training ---------------------------------------------------------------------------------------------------------------
    def _act_train(self, featmap_nhwc, b, tg, memory, restart_batch, noise, state_ini):
        """ppo_continuous.py:78-109 with training=True: the action 1 - relu(1 - relu(mu + action_std * z)), z = `noise` (B, 2) standard
        normals (None: torch.randn on the device, one draw per step), its log-probability, and the memory filled as the reference fills
        it (states: `state_ini`, or the (B, Tg*C, h, w) view of the dense pixel-major state)."""
        self._need_train_mode("act(training=True)")
        _, hh, ww, ch = featmap_nhwc.shape
        dev = featmap_nhwc.device
        if self.with_bn and b < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((b, self.hidden_state_dim),))
        # the channel-concatenated state, pixel-major: channel index tg * C + c as in the reference's view
        dense = featmap_nhwc.view(b, tg, hh, ww, ch).permute(0, 2, 3, 1, 4).reshape(b, hh, ww, tg * ch)
        fwd = self._encode_train(dense)
        if restart_batch:
            del memory.hidden[:]
            memory.hidden.append(torch.zeros(1, b, self.hidden_state_dim, device=dev))
        g, actor = self.gru, self.actor[0]
        hs = hip_ops.gru_seq_forward(fwd["e"].view(b, 1, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(), g.bias_ih_l0.detach(),
                                     g.bias_hh_l0.detach(), h0=memory.hidden[-1].view(b, -1))
        memory.hidden.append(hs.view(1, b, -1))
        mu = hip_ops.linear(hs.view(b, -1), actor.weight.detach(), actor.bias.detach(), act=hip_ops.ACT_SIGMOID)
        if noise is None:
            noise = torch.randn(b, 2, device=dev, dtype=torch.float32)
        action, logprob = hip_ops.ppo_gauss_sample(mu, noise, self.action_std)
        memory.states.append(state_ini if state_ini is not None else dense.permute(0, 3, 1, 2))
        memory.actions.append(action)
        memory.logprobs.append(logprob)
        return action

    def _evaluate_actions(self, action):
        return action.detach().float()

    def _head_stats(self, head, actions):
        return hip_ops.ppo_gauss_head_stats(head, actions, self.action_std)

    def _head_backward(self, head, actions, g_logprob, g_value, g_entropy):
        return hip_ops.ppo_gauss_head_backward(head, actions, self.action_std, g_logprob, g_value)

    def _loss_head(self, head, actions, old_logprobs, returns, eps_clip):
        return hip_ops.ppo_gauss_loss_head(head, actions, self.action_std, old_logprobs, returns, eps_clip)


class PPO_Continuous:
    """Plain holder (not an nn.Module, like the reference: its weights live under the checkpoint's
    separate 'policy' key, STH/evaluate.py:142-146) of policy / policy_old, the optimizer and the PPO update of stage 2."""

    def __init__(self, feature_dim, state_dim, hidden_state_dim, policy_conv, gpu=0, lr=0.0003, betas=(0.9, 0.999),
                 gamma=0.7, K_epochs=1, eps_clip=0.2, action_std=0.1, with_bn=False):
        self.lr, self.betas, self.gamma, self.eps_clip, self.K_epochs = lr, betas, gamma, eps_clip, K_epochs
        self.policy = ActorCritic(feature_dim, state_dim, hidden_state_dim, policy_conv, action_std, with_bn)
        self.optimizer = torch.optim.Adam(self.policy.parameters(), lr=lr, betas=betas)
        self.policy_old = ActorCritic(feature_dim, state_dim, hidden_state_dim, policy_conv, action_std, with_bn)
        self.policy_old.load_state_dict(self.policy.state_dict())
        self.last_loss = None

    def to(self, device):
        self.policy.to(device)
        self.policy_old.to(device)
        return self

    def select_action(self, state, memory, restart_batch=False, training=True):
        return self.policy_old.act(state, memory, restart_batch, training)

    def update(self, memory):
        """ppo_continuous.py:165-196 (policy_train.ppo_update).  `last_loss` keeps the last epoch's loss.mean() (a device tensor)."""
        loss = ppo_update(self.policy, self.policy_old, self.optimizer, memory, self.gamma, self.eps_clip, self.K_epochs)
        if loss is not None:
            self.last_loss = loss
