"""Stage-2 training core of both patch-location policies: the discrete one of ``ppo.py`` and the continuous one of
``ppo_continuous.py`` are the same network up to the action distribution -- state encoder (1x1 conv -> [BatchNorm2d] ReLU -> flatten ->
Linear -> [BatchNorm1d] ReLU), GRU, actor and critic Linear stacked into one head -- and so is their PPO update.

``PolicyTrainMixin`` is the base of both ``ActorCritic`` classes: the engine-layout weight cache, the training forward that keeps the
activations, the HIP backward for every policy parameter and ``evaluate`` through ``PolicyEvaluateFn``.  ``ppo_update`` is the update
both ``PPO.update`` and ``PPO_Continuous.update`` run: returns kernel -> K_epochs x {forward, loss head, backward, Adam step} ->
policy_old <- policy.  The Linear state encoder (``policy_conv=False``) has no backward here: ``evaluate`` / ``update`` raise.

A policy class supplies its distribution -- ``_head_stats`` / ``_head_backward`` / ``_loss_head`` (the three modes of the head kernel of
csrc/ppo_train.hip), ``_evaluate_actions`` (the stored actions in the dtype and shape its head kernel reads) and ``entropy_has_grad`` --
and ``needs_train_mode``."""
import torch
from torch import nn

from . import hip_ops

__all__ = ["PolicyTrainMixin", "PolicyEvaluateFn", "ppo_update"]

_FWD_TENSORS = ("states", "e1", "e_bt", "gi", "hs", "head", "head_w", "w_ih", "w_hh", "b_hh", "w_lin")
_BN_TENSORS = ("c1", "gamma1", "mean1", "invstd1", "l1", "gamma2", "mean2", "invstd2")


class PolicyTrainMixin:
    entropy_has_grad = True        # False: the entropy is a constant of the distribution (marked non-differentiable)
    needs_train_mode = False       # True: the training paths refuse a module in eval mode (BatchNorm would not use batch statistics)

    @property
    def with_bn(self):
        return isinstance(self.state_encoder[1], nn.BatchNorm2d)

    def _need_conv_encoder(self):
        if not self.policy_conv:
            raise NotImplementedError("the Linear state encoder (policy_conv=False) has no HIP backward: evaluate / update are implemented "
                                      "for the 1x1-conv encoder only")

    def _need_train_mode(self, what):
        if self.needs_train_mode and not self.training:
            raise NotImplementedError("%s is stage-2 (PPO) training: call model.policy_train_mode() first (this policy is in eval mode, "
                                      "where BatchNorm would not use batch statistics)" % what)

    def _evaluate_actions(self, action):
        return action

    def _hip_weights(self, hw):
        """Engine-layout views of the conv and Linear weights (cached on the parameter versions): the conv filter as (cmid, 1, 1, C), the
        Linear weight with pixel-major columns (the reference flattens (B, cmid, h, w) channel-major; the engine's map is pixel-major)."""
        conv, lin = self.state_encoder[0], self.state_encoder[4 if self.with_bn else 3]
        sig = tuple((q.data_ptr(), q._version) for q in (conv.weight, lin.weight)) + (hw,)
        if getattr(self, "_hipw_sig", None) != sig:
            cmid = conv.weight.shape[0]
            w_enc = conv.weight.detach().reshape(cmid, 1, 1, -1).contiguous()
            w_lin = lin.weight.detach().view(-1, cmid, hw).permute(0, 2, 1).reshape(lin.weight.shape[0], hw * cmid).contiguous()
            self._hipw, self._hipw_sig = (w_enc, w_lin), sig
        return self._hipw

    def _states_dense(self, state):
        """(T, B, C, h, w) [reference layout, or the permuted view of a pixel-major state] or (T, B, h, w, C) -> contiguous
        (T, B, h, w, C); C = feature_dim (Tg * 1280 channel-concatenated for the continuous policy)."""
        if state.shape[2] == self.feature_dim and state.shape[-1] != self.feature_dim:
            state = state.permute(0, 1, 3, 4, 2)
        return state.contiguous()

    _states_nhwc = _states_dense

    def _bn_forward(self, bn, x):
        """BatchNorm with batch statistics + ReLU over the rows of x, as the module in train mode does it: running statistics and
        num_batches_tracked move."""
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("BatchNorm with momentum=None, without running statistics or without affine parameters")
        out = hip_ops.bn_train_forward(x, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, bn.momentum)
        bn.num_batches_tracked += 1
        return out

    def _encode_train(self, dense):
        """The state encoder over dense pixel-major states (N, h, w, C), keeping what the backward needs: dict with e1 (N, h*w*cmid) and
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

    def _train_forward(self, states_dense):
        """The policy over a stored roll-out, keeping what the backward needs: states (T, B, h, w, C) -> dict with the stacked head
        output `head` (B*T, A + 1) [actor logits | critic value], rows b * T + t."""
        self._need_conv_encoder()
        self._need_train_mode("evaluate / update")
        t, b, hh, ww, c = states_dense.shape
        n = t * b
        if self.with_bn and n < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((n, self.hidden_state_dim),))
        s = states_dense.view(n, hh, ww, c)
        fwd = self._encode_train(s)                                                         # rows t * B + b
        e_bt = hip_ops.rows_transpose(fwd.pop("e"), t, b)                                   # rows b * T + t
        head_w = torch.cat([self.actor[0].weight.detach(), self.critic[0].weight.detach()], 0)
        head_b = torch.cat([self.actor[0].bias.detach(), self.critic[0].bias.detach()], 0)
        g = self.gru
        w = [p.detach() for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
        head, gi, hs = hip_ops.gru_cls_train_forward(e_bt.view(b, t, -1), w[0], w[1], w[2], w[3], head_w, head_b, None)
        fwd.update(states=s, e_bt=e_bt, gi=gi, hs=hs, head=head, head_w=head_w, w_ih=w[0], w_hh=w[1], b_hh=w[3], t=t, b=b)
        return fwd

    def _train_backward(self, fwd, dhead):
        """Gradients of every policy parameter from d loss / d head (B*T, A + 1): {name: tensor} in the parameters' own layouts."""
        t, b = fwd["t"], fwd["b"]
        x = fwd["e_bt"].view(b, t, -1)
        dx, dw_ih, dw_hh, db_ih, db_hh, dw_head, db_head = hip_ops.gru_cls_backward(x, fwd["w_ih"], fwd["w_hh"], fwd["b_hh"], fwd["head_w"],
                                                                                    fwd["gi"], fwd["hs"], None, dhead, want_dx=True)
        bn = tuple(fwd[k] for k in _BN_TENSORS) if self.with_bn else None
        out = hip_ops.ppo_encoder_backward(fwd["states"], fwd["e1"], fwd["e_bt"], dx, t, b, fwd["w_lin"], bn)
        lin = 4 if self.with_bn else 3
        a = dw_head.shape[0] - 1
        grads = {"state_encoder.0.weight": out[0].view(out[0].shape[0], -1, 1, 1), "state_encoder.%d.weight" % lin: out[1],
                 "state_encoder.%d.bias" % lin: out[2], "gru.weight_ih_l0": dw_ih, "gru.weight_hh_l0": dw_hh, "gru.bias_ih_l0": db_ih,
                 "gru.bias_hh_l0": db_hh, "actor.0.weight": dw_head[:a], "actor.0.bias": db_head[:a], "critic.0.weight": dw_head[a:],
                 "critic.0.bias": db_head[a:]}
        if self.with_bn:
            grads.update({"state_encoder.1.weight": out[3], "state_encoder.1.bias": out[4], "state_encoder.5.weight": out[5],
                          "state_encoder.5.bias": out[6]})
        return grads

    def evaluate(self, state, action):
        """ppo.py:98-122 / ppo_continuous.py:111-139: state (T, B, C, h, w) (or its pixel-major form), action (T, B) int64 or (T, B, 2)
        -> (logprobs, state values, entropy), each (T, B), differentiable with respect to every policy parameter (HIP forward and
        backward)."""
        self._need_conv_encoder()
        return PolicyEvaluateFn.apply(self, self._states_dense(state), self._evaluate_actions(action),
                                      *(p for _, p in self.named_parameters()))


class PolicyEvaluateFn(torch.autograd.Function):
    """ActorCritic.evaluate with a HIP backward: apply(policy, states (T, B, h, w, C), actions, *parameters in named_parameters() order)
    -> (logprobs, values, entropy).  The parameters are inputs only so that autograd routes their gradients; the forward reads them from
    the module as they are (nothing cached across calls but the engine-layout weight views, which key on the parameter versions).  The
    activations and the weight views the backward reads go through save_for_backward, so a parameter changed in place between evaluate
    and backward (an optimizer step) is an autograd error, not a silently mixed gradient.  The states are data: they get no gradient."""

    @staticmethod
    def forward(ctx, policy, states, actions, *params):
        fwd = policy._train_forward(states)
        keys = _FWD_TENSORS + (_BN_TENSORS if policy.with_bn else ())
        ctx.policy, ctx.dims, ctx.keys = policy, (fwd["t"], fwd["b"]), keys
        ctx.save_for_backward(actions, *(fwd[k] for k in keys))
        out = policy._head_stats(fwd["head"], actions)
        if not policy.entropy_has_grad:
            ctx.mark_non_differentiable(out[2])
        return out

    @staticmethod
    def backward(ctx, g_logprob, g_value, g_entropy):
        actions, *tensors = ctx.saved_tensors
        policy = ctx.policy
        fwd = dict(zip(ctx.keys, tensors), t=ctx.dims[0], b=ctx.dims[1])
        if not policy.entropy_has_grad:
            g_entropy = None
        dhead = policy._head_backward(fwd["head"], actions, *(None if g is None else g.float() for g in (g_logprob, g_value, g_entropy)))
        grads = policy._train_backward(fwd, dhead)
        return (None, None, None) + tuple(grads[n] for n, _ in policy.named_parameters())


def ppo_update(policy, policy_old, optimizer, memory, gamma, eps_clip, K_epochs):
    """ppo.py:147-178 / ppo_continuous.py:165-196: discounted, normalised returns; K_epochs x {policy forward over the stored roll-out,
    PPO loss head with its gradient, HIP backward, Adam step}; then policy_old <- policy, BatchNorm buffers included.  Returns the last
    epoch's loss.mean() (a device tensor; None when K_epochs is 0)."""
    policy._need_conv_encoder()
    policy._need_train_mode("update")
    rewards = torch.cat([r.reshape(1, -1) for r in memory.rewards], 0).float()
    returns = hip_ops.ppo_returns(rewards, gamma)
    # the stacked states laid out once as dense pixel-major (T, B, h, w, C): the one large copy of the update
    dense = [s.permute(0, 2, 3, 1) if s.shape[1] == policy.feature_dim and s.shape[-1] != policy.feature_dim else s for s in memory.states]
    states = policy._states_dense((dense[0][None] if len(dense) == 1 else torch.stack(dense, 0)).detach())
    actions = torch.stack(memory.actions, 0).detach()
    old_logprobs = torch.stack(memory.logprobs, 0).detach()
    params = dict(policy.named_parameters())
    loss = None
    with torch.no_grad():
        for _ in range(K_epochs):
            fwd = policy._train_forward(states)
            _, _, _, loss, dhead = policy._loss_head(fwd["head"], actions, old_logprobs, returns, eps_clip)
            grads = policy._train_backward(fwd, dhead)
            for n, g in grads.items():
                params[n].grad = g.contiguous()
            optimizer.step()
    policy_old.load_state_dict(policy.state_dict())
    return loss
