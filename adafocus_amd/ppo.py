"""Patch-location policy (ACT/models/ppo.py): the inference branch, the sampling roll-out and the PPO update of stage 2.

The policy is the PRODUCER of the crop coordinates; its output tensor is handed
to the HIP gather without a host round trip.

Stage-2 training: ``act(training=True)`` samples from the actor's softmax with caller-drawn uniforms
(csrc/ppo_train.hip), ``evaluate`` is the policy forward over a stored roll-out through ``PolicyEvaluateFn`` (HIP forward that keeps the
activations, HIP backward for every policy parameter) and ``PPO.update`` runs returns kernel -> K_epochs x {forward, loss head, backward,
Adam step}.  The GRU with both heads is the stage-3 GRU + Linear pair with the actor and critic weights stacked into one (A + 1)-row
Linear.  The Linear state encoder (``policy_conv=False``) has no backward here: its ``evaluate`` / ``update`` raise.

``ActorCritic.act_rollout_nhwc`` is the sampling roll-out of all T steps at once (the policy's input never contains local features): it
leaves the memory as T calls of ``act(training=True)`` leave it and returns the crop coordinates in the trunk's row order.

``ActorCritic.act_sequence_nhwc`` is the offline-inference form on the HIP engine: in eval mode the
policy input is only the glancer feature map and its own hidden state (ppo.py:67-96), so all T
actions are computed before any patch is cropped -- 1x1 conv + Linear over all B*T frames at once,
one GRU scan, one actor GEMM, arg-max + table lookup in one small kernel.  ``act`` (one step,
reference signature, hidden state carried in ``memory.hidden`` element for element like the reference: the zero
state after `restart_batch`, then one entry per step) runs the same kernels with T = 1 and ``h0`` = the previous
step's state; both encoders (`policy_conv` True / False) run on the engine; nothing on this surface is an ATen / MIOpen op.
"""
import torch
from torch import nn

from . import hip_ops

__all__ = ["Memory", "ActorCritic", "PPO", "PolicyEvaluateFn"]

PARAM_NAMES = ("state_encoder.0.weight", "state_encoder.3.weight", "state_encoder.3.bias", "gru.weight_ih_l0", "gru.weight_hh_l0",
               "gru.bias_ih_l0", "gru.bias_hh_l0", "actor.0.weight", "actor.0.bias", "critic.0.weight", "critic.0.bias")


class Memory:
    def __init__(self):
        self.actions, self.states, self.logprobs, self.rewards, self.is_terminals, self.hidden = [], [], [], [], [], []

    def clear_memory(self):
        for lst in (self.actions, self.states, self.logprobs, self.rewards, self.is_terminals, self.hidden):
            del lst[:]


class ActorCritic(nn.Module):
    def __init__(self, feature_dim, state_dim, action_dim, hidden_state_dim=1024, policy_conv=True):
        super().__init__()
        if policy_conv:
            self.state_encoder = nn.Sequential(
                nn.Conv2d(feature_dim, 32, 1, bias=False), nn.ReLU(), nn.Flatten(),
                nn.Linear(int(state_dim * 32 / feature_dim), hidden_state_dim), nn.ReLU())
        else:
            self.state_encoder = nn.Sequential(nn.Linear(state_dim, 2048), nn.ReLU(),
                                               nn.Linear(2048, hidden_state_dim), nn.ReLU())
        self.gru = nn.GRU(hidden_state_dim, hidden_state_dim, batch_first=False)
        self.actor = nn.Sequential(nn.Linear(hidden_state_dim, action_dim), nn.Softmax(dim=-1))
        self.critic = nn.Sequential(nn.Linear(hidden_state_dim, 1))
        self.hidden_state_dim, self.action_dim, self.policy_conv, self.feature_dim = \
            hidden_state_dim, action_dim, policy_conv, feature_dim

    def act(self, state_ini, memory, restart_batch=False, training=True, uniforms=None):
        """One step of ppo.py:67-96.  training=False: arg-max of the actor's softmax.  training=True: a sample from it -- the first index
        whose running sum of probabilities exceeds `uniforms` (B,) in [0, 1), drawn with torch.rand on the device when None --, with the
        state, the action and its log-probability appended to `memory` (ppo.py:87-92)."""
        b = state_ini.size(0)
        if restart_batch:
            # ppo.py:68-70: the list restarts with the zero state, so memory.hidden holds k + 1 entries after k steps
            del memory.hidden[:]
            memory.hidden.append(torch.zeros(1, b, self.hidden_state_dim, device=state_ini.device))
        e = self._encode(state_ini)
        g, actor = self.gru, self.actor[0]
        hs = hip_ops.gru_seq_forward(e.view(b, 1, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(),
                                     g.bias_ih_l0.detach(), g.bias_hh_l0.detach(), h0=memory.hidden[-1].view(b, -1))
        memory.hidden.append(hs.view(1, b, -1))
        logits = hip_ops.linear(hs.view(b, -1), actor.weight.detach(), actor.bias.detach())
        if not training:
            return hip_ops.argmax_rows(logits)
        if uniforms is None:
            uniforms = torch.rand(b, device=state_ini.device, dtype=torch.float32)
        action, logprob = hip_ops.ppo_sample(logits, uniforms)
        memory.states.append(state_ini)
        memory.actions.append(action)
        memory.logprobs.append(logprob)
        return action

    def _states_nhwc(self, state):
        """(T, B, C, h, w) [reference layout, or the permuted view of a pixel-major map] or (T, B, h, w, C) -> contiguous (T, B, h, w, C)."""
        if state.shape[2] == self.feature_dim and state.shape[-1] != self.feature_dim:
            state = state.permute(0, 1, 3, 4, 2)
        return state.contiguous()

    def _train_forward(self, states_nhwc):
        """The policy over a stored roll-out, keeping what the backward needs: states (T, B, h, w, C) -> dict with the stacked head output
        `head` (B*T, A + 1) [actor logits | critic value], rows b * T + t."""
        if not self.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        t, b, hh, ww, c = states_nhwc.shape
        n, hw = t * b, hh * ww
        w_enc, w_lin = self._hip_weights(hw)
        g = self.gru
        s = states_nhwc.view(n, hh, ww, c)
        e1 = hip_ops.conv2d_bn_act(s, w_enc, act=hip_ops.ACT_RELU)                                                   # (T*B, h, w, 32)
        e = hip_ops.linear(e1.view(n, -1), w_lin, self.state_encoder[3].bias.detach(), act=hip_ops.ACT_RELU)          # rows t * B + b
        e_bt = hip_ops.rows_transpose(e, t, b)                                                                       # rows b * T + t
        head_w = torch.cat([self.actor[0].weight.detach(), self.critic[0].weight.detach()], 0)
        head_b = torch.cat([self.actor[0].bias.detach(), self.critic[0].bias.detach()], 0)
        w = [p.detach() for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
        head, gi, hs = hip_ops.gru_cls_train_forward(e_bt.view(b, t, -1), w[0], w[1], w[2], w[3], head_w, head_b, None)
        return dict(states=s, e1=e1, e_bt=e_bt, gi=gi, hs=hs, head=head, head_w=head_w, w_ih=w[0], w_hh=w[1], b_hh=w[3], w_lin=w_lin,
                    t=t, b=b)

    def _train_backward(self, fwd, dhead):
        """Gradients of every policy parameter from d loss / d head (B*T, A + 1): {name: tensor} in the parameters' own layouts."""
        t, b = fwd["t"], fwd["b"]
        x = fwd["e_bt"].view(b, t, -1)
        dx, dw_ih, dw_hh, db_ih, db_hh, dw_head, db_head = hip_ops.gru_cls_backward(x, fwd["w_ih"], fwd["w_hh"], fwd["b_hh"], fwd["head_w"],
                                                                                    fwd["gi"], fwd["hs"], None, dhead, want_dx=True)
        dw_enc, dw_lin, db_lin = hip_ops.ppo_encoder_backward(fwd["states"], fwd["e1"].view(t * b, -1), fwd["e_bt"], dx, t, b, fwd["w_lin"])
        a = self.action_dim
        return dict(zip(PARAM_NAMES, (dw_enc.view(dw_enc.shape[0], -1, 1, 1), dw_lin, db_lin, dw_ih, dw_hh, db_ih, db_hh,
                                      dw_head[:a], db_head[:a], dw_head[a:], db_head[a:])))

    def evaluate(self, state, action):
        """ppo.py:98-122: state (T, B, C, h, w) (or its pixel-major form), action (T, B) int64 -> (logprobs, state values, entropy), each
        (T, B), differentiable with respect to every policy parameter (HIP forward and backward)."""
        if not self.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        params = dict(self.named_parameters())
        return PolicyEvaluateFn.apply(self, self._states_nhwc(state), action, *(params[n] for n in PARAM_NAMES))

    def _encode(self, state):
        """state_encoder on the engine.  policy_conv=True (ppo.py:31-39: MobileNet / EfficientNet / RegNet feature maps):
        1x1 conv + ReLU + flatten + Linear + ReLU over (N, C, h, w) [reference layout] or (N, h, w, C) [pixel-major];
        policy_conv=False (ppo.py:40-47: ResNet / DenseNet features): `state.flatten(1)` through two Linear + ReLU."""
        n = state.shape[0]
        if not self.policy_conv:
            l0, l1 = self.state_encoder[0], self.state_encoder[2]
            e = hip_ops.linear(state.reshape(n, -1).contiguous(), l0.weight.detach(), l0.bias.detach(), act=hip_ops.ACT_RELU)
            return hip_ops.linear(e, l1.weight.detach(), l1.bias.detach(), act=hip_ops.ACT_RELU)
        # (B, C, h, w) reference layout -> pixel-major; free when `state` is a permuted view of the HIP glancer's map
        nhwc = state.permute(0, 2, 3, 1).contiguous() if state.shape[1] == self.feature_dim and state.shape[-1] != self.feature_dim else state
        hw = nhwc.shape[1] * nhwc.shape[2]
        w_enc, w_lin = self._hip_weights(hw)
        lin = self.state_encoder[3]
        e = hip_ops.conv2d_bn_act(nhwc, w_enc, act=hip_ops.ACT_RELU)
        return hip_ops.linear(e.view(n, -1), w_lin, lin.bias.detach(), act=hip_ops.ACT_RELU)

    def _hip_weights(self, hw):
        """Engine-layout views of the parameters (cached on the parameter versions)."""
        enc, lin = self.state_encoder[0], self.state_encoder[3]
        sig = tuple((q.data_ptr(), q._version) for q in (enc.weight, lin.weight))
        if getattr(self, "_hipw_sig", None) != sig:
            cmid = enc.weight.shape[0]
            w_enc = enc.weight.detach().reshape(cmid, 1, 1, -1).contiguous()
            # reference flattens (B, cmid, h, w) channel-major; the engine's map is pixel-major
            w_lin = lin.weight.detach().view(-1, cmid, hw).permute(0, 2, 1).reshape(lin.weight.shape[0], hw * cmid).contiguous()
            self._hipw, self._hipw_sig = (w_enc, w_lin), sig
        return self._hipw

    @torch.no_grad()
    def act_sequence_nhwc(self, featmap_nhwc, b, t, table):
        """featmap (B*T, h, w, C) pixel-major (the HIP glancer's output) -> (idx (B,T) int64,
        actions (B*T, 2) fp32 = table[idx])."""
        n = featmap_nhwc.shape[0]
        g, act = self.gru, self.actor[0]
        if self.policy_conv:
            e = self._encode(featmap_nhwc)                                                       # (n, 1024)
        else:   # the Linear encoder flattens the reference's (C, h, w) order
            e = self._encode(featmap_nhwc.permute(0, 3, 1, 2))
        hs = hip_ops.gru_seq_forward(e.view(b, t, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(),
                                     g.bias_ih_l0.detach(), g.bias_hh_l0.detach())
        logits = hip_ops.linear(hs.view(b * t, -1), act.weight.detach(), act.bias.detach())
        idx, actions = hip_ops.grid_actions(logits, table)
        return idx.view(b, t), actions

    @torch.no_grad()
    def act_rollout_nhwc(self, featmap_nhwc, b, t, memory, table, uniforms=None):
        """The sampling roll-out of stage-2 training in one pass: T calls of ``act(training=True)`` (the first with restart_batch) on the
        steps of featmap (B*T, h, w, C) pixel-major, frames b * T + t.  Encoder over all B*T frames, one GRU scan, one actor GEMM, one
        sampling launch; `memory` is left exactly as the T calls leave it (states: the (B, C, h, w) views of the map; actions, logprobs:
        T tensors (B,); hidden: the zero state and T entries (1, B, H)).  uniforms (T, B) in [0, 1); None draws torch.rand(B) on the device
        T times in step order, the loop's draw sequence.  Returns (actions (T, B) int64, coords (B*T, 2) fp32 = table[action], rows
        b * T + t: what the frame-gathering trunk pass reads)."""
        dev = featmap_nhwc.device
        g, act = self.gru, self.actor[0]
        if self.policy_conv:
            e = self._encode(featmap_nhwc)
        else:   # the Linear encoder flattens the reference's (C, h, w) order
            e = self._encode(featmap_nhwc.permute(0, 3, 1, 2))
        hs = hip_ops.gru_seq_forward(e.view(b, t, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(),
                                     g.bias_ih_l0.detach(), g.bias_hh_l0.detach())
        logits = hip_ops.linear(hs.view(b * t, -1), act.weight.detach(), act.bias.detach())
        if uniforms is None:
            uniforms = torch.stack([torch.rand(b, device=dev, dtype=torch.float32) for _ in range(t)], 0)
        actions, logprobs, coords = hip_ops.ppo_sample_actions(logits, uniforms, table)
        steps = featmap_nhwc.unflatten(0, (b, t))
        hs_tb = hs.transpose(0, 1).contiguous()
        del memory.hidden[:]
        memory.hidden.append(torch.zeros(1, b, self.hidden_state_dim, device=dev))
        for s in range(t):
            memory.states.append(steps[:, s].permute(0, 3, 1, 2))
            memory.actions.append(actions[s])
            memory.logprobs.append(logprobs[s])
            memory.hidden.append(hs_tb[s:s + 1])
        return actions, coords


_FWD_TENSORS = ("states", "e1", "e_bt", "gi", "hs", "head", "head_w", "w_ih", "w_hh", "b_hh", "w_lin")


class PolicyEvaluateFn(torch.autograd.Function):
    """ActorCritic.evaluate with a HIP backward: apply(policy, states (T,B,h,w,C), actions (T,B), *parameters in PARAM_NAMES order) ->
    (logprobs, values, entropy).  The parameters are inputs only so that autograd routes their gradients; the forward reads them from the
    module as they are (nothing cached across calls but the engine-layout weight views, which key on the parameter versions).  The
    activations and the weight views the backward reads go through save_for_backward, so a parameter changed in place between evaluate
    and backward (an optimizer step) is an autograd error, not a silently mixed gradient.  The states are data: they get no gradient."""

    @staticmethod
    def forward(ctx, policy, states, actions, *params):
        fwd = policy._train_forward(states)
        ctx.policy, ctx.dims = policy, (fwd["t"], fwd["b"])
        ctx.save_for_backward(actions, *(fwd[k] for k in _FWD_TENSORS))
        return hip_ops.ppo_head_stats(fwd["head"], actions)

    @staticmethod
    def backward(ctx, g_logprob, g_value, g_entropy):
        actions, *tensors = ctx.saved_tensors
        fwd = dict(zip(_FWD_TENSORS, tensors), t=ctx.dims[0], b=ctx.dims[1])
        dhead = hip_ops.ppo_head_backward(fwd["head"], actions, *(None if g is None else g.float() for g in (g_logprob, g_value, g_entropy)))
        grads = ctx.policy._train_backward(fwd, dhead)
        return (None, None, None) + tuple(grads[n] for n in PARAM_NAMES)


class PPO(nn.Module):
    """policy / policy_old with the reference's attribute and state-dict names, and the PPO update of stage 2."""

    def __init__(self, feature_dim, state_dim, action_dim, hidden_state_dim, policy_conv, gpu=0, lr=0.0003,
                 betas=(0.9, 0.999), gamma=0.7, K_epochs=1, eps_clip=0.2):
        super().__init__()
        self.lr, self.betas, self.gamma, self.eps_clip, self.K_epochs = lr, betas, gamma, eps_clip, K_epochs
        self.policy = ActorCritic(feature_dim, state_dim, action_dim, hidden_state_dim, policy_conv)
        self.policy_old = ActorCritic(feature_dim, state_dim, action_dim, hidden_state_dim, policy_conv)
        self.policy_old.load_state_dict(self.policy.state_dict())
        # (ppo.py:137; a plain attribute: the module's state-dict keys do not change)
        self.optimizer = torch.optim.Adam(self.policy.parameters(), lr=lr, betas=betas)
        self.last_loss = None

    def select_action(self, state, memory, restart_batch=False, training=True):
        return self.policy_old.act(state, memory, restart_batch, training)

    def update(self, memory):
        """ppo.py:147-178: discounted, normalised returns; K_epochs x {policy forward over the stored roll-out, PPO loss head with its
        gradient, HIP backward, Adam step}; then policy_old <- policy.  `last_loss` keeps the last epoch's loss.mean() (a device tensor)."""
        pol = self.policy
        if not pol.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")
        rewards = torch.cat([r.reshape(1, -1) for r in memory.rewards], 0).float()
        returns = hip_ops.ppo_returns(rewards, self.gamma)
        states = torch.stack([s.permute(0, 2, 3, 1) if s.shape[1] == pol.feature_dim and s.shape[-1] != pol.feature_dim else s
                              for s in memory.states], 0).detach()                          # (T, B, h, w, C)
        actions = torch.stack(memory.actions, 0).detach()
        old_logprobs = torch.stack(memory.logprobs, 0).detach()
        params = dict(pol.named_parameters())
        with torch.no_grad():
            for _ in range(self.K_epochs):
                fwd = pol._train_forward(states)
                _, _, _, loss, dhead = hip_ops.ppo_loss_head(fwd["head"], actions, old_logprobs, returns, self.eps_clip)
                grads = pol._train_backward(fwd, dhead)
                for n, g in grads.items():
                    params[n].grad = g.contiguous()
                self.optimizer.step()
                self.last_loss = loss
        self.policy_old.load_state_dict(self.policy.state_dict())
