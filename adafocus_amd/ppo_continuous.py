"""Continuous patch-location policy (STH/models/ppo_continuous.py): encoder -> GRU step -> Linear(2) + Sigmoid, the producer of the (y, x)
fractions the HIP gather consumes, on the conv engine + the GRU kernel; the hidden state is carried across
``video_div`` steps in ``memory.hidden`` like the reference does.

Inference (``training=False``): the action is the mean; BatchNorm is folded from the running statistics (the reference's eval branch
still draws ``dist.sample()`` and discards it, ppo_continuous.py:98,107 -- it only advances the global RNG).

Stage-2 training (the module in train mode, ``GFV.policy_train_mode()``): ``act(training=True)`` samples
``1 - relu(1 - relu(mu + sigma z))`` from caller-drawn normals and stores state, action and log-probability; ``evaluate`` is the policy
forward over a stored roll-out through ``PolicyEvaluateFn`` (HIP forward that keeps the activations, HIP backward for every policy
parameter); ``PPO_Continuous.update`` runs returns kernel -> K_epochs x {forward, Gaussian loss head, backward, Adam step}.  BatchNorm
uses batch statistics on these paths (a roll-out step over B rows, evaluate over T*B rows) and updates the running ones.  ``action_std``
is the standard deviation itself: the reference hands ``diag(action_var)`` to MultivariateNormal as ``scale_tril``."""
import torch
from torch import nn

from . import hip_ops
from .ppo import Memory  # noqa: F401  (same class in both reference files)

__all__ = ["ActorCritic", "PPO_Continuous", "Memory"]


class ActorCritic(nn.Module):
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
    @property
    def with_bn(self):
        return isinstance(self.state_encoder[1], nn.BatchNorm2d)

    def _need_train_mode(self, what):
        if not self.training:
            raise NotImplementedError("%s is stage-2 (PPO) training: call model.policy_train_mode() first (this policy is in eval mode, "
                                      "where BatchNorm would not use batch statistics)" % what)

    def _hip_weights(self, hw):
        """Engine-layout views of the conv and Linear weights (cached on the parameter versions): the conv filter as (64, 1, 1, Tg*C), the
        Linear weight with pixel-major columns (the reference flattens (B, 64, h, w) channel-major)."""
        conv, lin = self.state_encoder[0], self.state_encoder[4 if self.with_bn else 3]
        sig = tuple((q.data_ptr(), q._version) for q in (conv.weight, lin.weight)) + (hw,)
        if getattr(self, "_hipw_sig", None) != sig:
            cmid = conv.weight.shape[0]
            w_enc = conv.weight.detach().reshape(cmid, 1, 1, -1).contiguous()
            w_lin = lin.weight.detach().view(-1, cmid, hw).permute(0, 2, 1).reshape(lin.weight.shape[0], hw * cmid).contiguous()
            self._hipw, self._hipw_sig = (w_enc, w_lin), sig
        return self._hipw

    def _bn_forward(self, bn, x):
        """BatchNorm with batch statistics + ReLU over the rows of x, as the module in train mode does it: running statistics and
        num_batches_tracked move."""
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("BatchNorm with momentum=None, without running statistics or without affine parameters")
        out = hip_ops.bn_train_forward(x, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, bn.momentum)
        bn.num_batches_tracked += 1
        return out

    def _encode_train(self, dense):
        """The state encoder over dense pixel-major states (N, h, w, Tg*C), keeping what the backward needs: dict with e1 (N, h*w*64) and
        e (N, hidden) after ReLU; with BatchNorm also the raw outputs c1 / l1 and the statistics they were normalised with."""
        n, hh, ww, _ = dense.shape
        hw = hh * ww
        enc = self.state_encoder
        w_enc, w_lin = self._hip_weights(hw)
        if not self.with_bn:
            e1 = hip_ops.conv2d_bn_act(dense, w_enc, act=hip_ops.ACT_RELU)
            e = hip_ops.linear(e1.view(n, -1), w_lin, enc[3].bias.detach(), act=hip_ops.ACT_RELU)
            return dict(e1=e1.view(n, -1), e=e, w_lin=w_lin)
        cmid = w_enc.shape[0]
        c1 = hip_ops.conv2d_bn_act(dense, w_enc).view(n * hw, cmid)
        e1, mean1, invstd1 = self._bn_forward(enc[1], c1)
        l1 = hip_ops.linear(e1.view(n, -1), w_lin, enc[4].bias.detach())
        e, mean2, invstd2 = self._bn_forward(enc[5], l1)
        return dict(e1=e1.view(n, -1), e=e, w_lin=w_lin, c1=c1, mean1=mean1, invstd1=invstd1, l1=l1, mean2=mean2, invstd2=invstd2,
                    gamma1=enc[1].weight.detach(), gamma2=enc[5].weight.detach())

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

    def _states_dense(self, state):
        """(T, B, Tg*C, h, w) [reference layout, or the permuted view of a dense pixel-major state] or (T, B, h, w, Tg*C) -> contiguous
        (T, B, h, w, Tg*C)."""
        if state.shape[2] == self.feature_dim and state.shape[-1] != self.feature_dim:
            state = state.permute(0, 1, 3, 4, 2)
        return state.contiguous()

    def _train_forward(self, states_dense):
        """The policy over a stored roll-out, keeping what the backward needs: states (T, B, h, w, Tg*C) -> dict with the stacked head
        output `head` (B*T, 3) [mean logits | critic value], rows b * T + t."""
        if not self.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        self._need_train_mode("evaluate / update")
        t, b, hh, ww, c = states_dense.shape
        n = t * b
        if self.with_bn and n < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((n, self.hidden_state_dim),))
        s = states_dense.view(n, hh, ww, c)
        fwd = self._encode_train(s)                                                         # rows t * B + b
        e_bt = hip_ops.rows_transpose(fwd["e"], t, b)                                       # rows b * T + t
        head_w = torch.cat([self.actor[0].weight.detach(), self.critic[0].weight.detach()], 0)
        head_b = torch.cat([self.actor[0].bias.detach(), self.critic[0].bias.detach()], 0)
        g = self.gru
        w = [p.detach() for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
        head, gi, hs = hip_ops.gru_cls_train_forward(e_bt.view(b, t, -1), w[0], w[1], w[2], w[3], head_w, head_b, None)
        fwd.update(states=s, e_bt=e_bt, gi=gi, hs=hs, head=head, head_w=head_w, w_ih=w[0], w_hh=w[1], b_hh=w[3], t=t, b=b)
        del fwd["e"]
        return fwd

    def _train_backward(self, fwd, dhead):
        """Gradients of every policy parameter from d loss / d head (B*T, 3): {name: tensor} in the parameters' own layouts."""
        t, b = fwd["t"], fwd["b"]
        x = fwd["e_bt"].view(b, t, -1)
        dx, dw_ih, dw_hh, db_ih, db_hh, dw_head, db_head = hip_ops.gru_cls_backward(x, fwd["w_ih"], fwd["w_hh"], fwd["b_hh"], fwd["head_w"],
                                                                                    fwd["gi"], fwd["hs"], None, dhead, want_dx=True)
        bn = tuple(fwd[k] for k in _BN_TENSORS) if self.with_bn else None
        out = hip_ops.ppo_encoder_bn_backward(fwd["states"], fwd["e1"], fwd["e_bt"], dx, t, b, fwd["w_lin"], bn)
        lin = 4 if self.with_bn else 3
        grads = {"state_encoder.0.weight": out[0].view(out[0].shape[0], -1, 1, 1), "state_encoder.%d.weight" % lin: out[1],
                 "state_encoder.%d.bias" % lin: out[2], "gru.weight_ih_l0": dw_ih, "gru.weight_hh_l0": dw_hh, "gru.bias_ih_l0": db_ih,
                 "gru.bias_hh_l0": db_hh, "actor.0.weight": dw_head[:2], "actor.0.bias": db_head[:2], "critic.0.weight": dw_head[2:],
                 "critic.0.bias": db_head[2:]}
        if self.with_bn:
            grads.update({"state_encoder.1.weight": out[3], "state_encoder.1.bias": out[4], "state_encoder.5.weight": out[5],
                          "state_encoder.5.bias": out[6]})
        return grads

    def evaluate(self, state, action):
        """ppo_continuous.py:111-139: state (T, B, Tg*C, h, w) (or its dense pixel-major form), action (T, B, 2) -> (logprobs, state
        values, entropy), each (T, B), differentiable with respect to every policy parameter (HIP forward and backward).  The entropy is
        the constant 1 + log 2 pi + 2 log action_std."""
        if not self.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        return PolicyEvaluateFn.apply(self, self._states_dense(state), action.detach().float(), *(p for _, p in self.named_parameters()))


_BN_TENSORS = ("c1", "gamma1", "mean1", "invstd1", "l1", "gamma2", "mean2", "invstd2")
_FWD_TENSORS = ("states", "e1", "e_bt", "gi", "hs", "head", "head_w", "w_ih", "w_hh", "b_hh", "w_lin")


class PolicyEvaluateFn(torch.autograd.Function):
    """ActorCritic.evaluate with a HIP backward: apply(policy, states (T, B, h, w, Tg*C), actions (T, B, 2), *parameters in
    named_parameters() order) -> (logprobs, values, entropy).  As ppo.PolicyEvaluateFn: the parameters are inputs only so that autograd
    routes their gradients, the forward reads them from the module; activations and weight views go through save_for_backward."""

    @staticmethod
    def forward(ctx, policy, states, actions, *params):
        fwd = policy._train_forward(states)
        keys = _FWD_TENSORS + (_BN_TENSORS if policy.with_bn else ())
        ctx.policy, ctx.dims, ctx.keys = policy, (fwd["t"], fwd["b"]), keys
        ctx.save_for_backward(actions, *(fwd[k] for k in keys))
        out = hip_ops.ppo_gauss_head_stats(fwd["head"], actions, policy.action_std)
        ctx.mark_non_differentiable(out[2])
        return out

    @staticmethod
    def backward(ctx, g_logprob, g_value, g_entropy):
        actions, *tensors = ctx.saved_tensors
        policy = ctx.policy
        fwd = dict(zip(ctx.keys, tensors), t=ctx.dims[0], b=ctx.dims[1])
        dhead = hip_ops.ppo_gauss_head_backward(fwd["head"], actions, policy.action_std,
                                                *(None if g is None else g.float() for g in (g_logprob, g_value)))
        grads = policy._train_backward(fwd, dhead)
        return (None, None, None) + tuple(grads[n] for n, _ in policy.named_parameters())


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
        """ppo_continuous.py:165-196: discounted, normalised returns; K_epochs x {policy forward over the stored roll-out, Gaussian PPO
        loss head with its gradient, HIP backward, Adam step}; then policy_old <- policy, BatchNorm buffers included.  `last_loss` keeps
        the last epoch's loss.mean() (a device tensor)."""
        pol = self.policy
        if not pol.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        pol._need_train_mode("update")
        rewards = torch.cat([r.reshape(1, -1) for r in memory.rewards], 0).float()
        returns = hip_ops.ppo_returns(rewards, self.gamma)
        # the stacked states laid out once as dense pixel-major (T, B, h, w, Tg*C): the one large copy of the update
        dense = [s.permute(0, 2, 3, 1) if s.shape[1] == pol.feature_dim and s.shape[-1] != pol.feature_dim else s for s in memory.states]
        states = pol._states_dense((dense[0][None] if len(dense) == 1 else torch.stack(dense, 0)).detach())
        actions = torch.stack(memory.actions, 0).detach()
        old_logprobs = torch.stack(memory.logprobs, 0).detach()
        params = dict(pol.named_parameters())
        with torch.no_grad():
            for _ in range(self.K_epochs):
                fwd = pol._train_forward(states)
                _, _, _, loss, dhead = hip_ops.ppo_gauss_loss_head(fwd["head"], actions, pol.action_std, old_logprobs, returns, self.eps_clip)
                grads = pol._train_backward(fwd, dhead)
                for n, g in grads.items():
                    params[n].grad = g.contiguous()
                self.optimizer.step()
                self.last_loss = loss
        self.policy_old.load_state_dict(self.policy.state_dict())
