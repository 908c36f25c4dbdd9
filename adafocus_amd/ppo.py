"""Patch-location policy (ACT/models/ppo.py): the inference branch, the sampling roll-out and the PPO update of stage 2.

The policy is the PRODUCER of the crop coordinates; its output tensor is handed
to the HIP gather without a host round trip.

Stage-2 training: ``act(training=True)`` samples from the actor's softmax with caller-drawn uniforms
(csrc/ppo_train.hip).  ``evaluate`` and ``PPO.update`` are the training core of ``policy_train.py``, shared with the continuous policy,
with the categorical head: the policy forward over a stored roll-out through ``PolicyEvaluateFn`` (HIP forward that keeps the activations,
HIP backward for every policy parameter) and returns kernel -> K_epochs x {forward, loss head, backward, Adam step}.  The GRU with both
heads is the stage-3 GRU + Linear pair with the actor and critic weights stacked into one (A + 1)-row Linear.  The Linear state encoder
(``policy_conv=False``) has no backward: its ``evaluate`` / ``update`` raise.

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
from .policy_train import PolicyEvaluateFn, PolicyTrainMixin, ppo_update  # noqa: F401  (PolicyEvaluateFn: the name it had here)

__all__ = ["Memory", "ActorCritic", "PPO", "PolicyEvaluateFn"]

# the policy's named_parameters() order (policy_conv=True)
PARAM_NAMES = ("state_encoder.0.weight", "state_encoder.3.weight", "state_encoder.3.bias", "gru.weight_ih_l0", "gru.weight_hh_l0",
               "gru.bias_ih_l0", "gru.bias_hh_l0", "actor.0.weight", "actor.0.bias", "critic.0.weight", "critic.0.bias")


class Memory:
    def __init__(self):
        self.actions, self.states, self.logprobs, self.rewards, self.is_terminals, self.hidden = [], [], [], [], [], []

    def clear_memory(self):
        for lst in (self.actions, self.states, self.logprobs, self.rewards, self.is_terminals, self.hidden):
            del lst[:]


class ActorCritic(PolicyTrainMixin, nn.Module):
    """The training core is policy_train.PolicyTrainMixin's; this class supplies the categorical distribution over the action_dim crops
    (differentiable entropy, int64 actions (T, B)) and the inference / roll-out surfaces."""

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
        hs, logits = self._gru_logits(self._encode(state_ini), b, 1, h0=memory.hidden[-1].view(b, -1))
        memory.hidden.append(hs.view(1, b, -1))
        if not training:
            return hip_ops.argmax_rows(logits)
        if uniforms is None:
            uniforms = torch.rand(b, device=state_ini.device, dtype=torch.float32)
        action, logprob = hip_ops.ppo_sample(logits, uniforms)
        memory.states.append(state_ini)
        memory.actions.append(action)
        memory.logprobs.append(logprob)
        return action

    def _head_stats(self, head, actions):
        return hip_ops.ppo_head_stats(head, actions)

    def _head_backward(self, head, actions, g_logprob, g_value, g_entropy):
        return hip_ops.ppo_head_backward(head, actions, g_logprob, g_value, g_entropy)

    def _loss_head(self, head, actions, old_logprobs, returns, eps_clip):
        return hip_ops.ppo_loss_head(head, actions, old_logprobs, returns, eps_clip)

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

    def _encode_map(self, featmap_nhwc):
        """_encode over the HIP glancer's pixel-major map; the Linear encoder flattens the reference's (C, h, w) order."""
        return self._encode(featmap_nhwc if self.policy_conv else featmap_nhwc.permute(0, 3, 1, 2))

    def _gru_logits(self, e, b, t, h0=None):
        """GRU scan over e (B*T, H) [rows b * T + t] from h0 (None: zeros) + the actor's Linear -> (hs (B, T, H), logits (B*T, A))."""
        g, actor = self.gru, self.actor[0]
        hs = hip_ops.gru_seq_forward(e.view(b, t, -1), g.weight_ih_l0.detach(), g.weight_hh_l0.detach(),
                                     g.bias_ih_l0.detach(), g.bias_hh_l0.detach(), h0=h0)
        return hs, hip_ops.linear(hs.view(b * t, -1), actor.weight.detach(), actor.bias.detach())

    @torch.no_grad()
    def act_sequence_nhwc(self, featmap_nhwc, b, t, table):
        """featmap (B*T, h, w, C) pixel-major (the HIP glancer's output) -> (idx (B,T) int64,
        actions (B*T, 2) fp32 = table[idx])."""
        _, logits = self._gru_logits(self._encode_map(featmap_nhwc), b, t)
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
        hs, logits = self._gru_logits(self._encode_map(featmap_nhwc), b, t)
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
        """ppo.py:147-178 (policy_train.ppo_update).  `last_loss` keeps the last epoch's loss.mean() (a device tensor)."""
        loss = ppo_update(self.policy, self.policy_old, self.optimizer, memory, self.gamma, self.eps_clip, self.K_epochs)
        if loss is not None:
            self.last_loss = loss
