"""Stage-2 training loop body (ACT/main_dist.py:494-518, 574-581): the PPO roll-out over T focus steps and the policy update.

    model.policy_train_mode()                 # in place of the reference's model.train_mode(args) at train_stage == 2
    for images, target in loader:
        preds, loss = train_stage2_batch(model, images.cuda(), target[:, 0].cuda(), args)

``train_stage2_batch_fused`` is the same body with the roll-out as one batched pass (``GFV.rollout_act``: all T actions sampled first, one
trunk pass over the B*T crops) and the rewards from one kernel; same contract, same predictions.

``train_stage2_batch_sth`` is the loop body of the Something-Something tree (STH/stage2.py:233-270) with its continuous policy.

Both CNNs and the classifier stay frozen and run on the HIP path; only ``focuser.policy.policy`` learns (``PPO.update``: HIP forward and
backward, PyTorch's Adam step).

``train_stage3_batch_sth`` is the stage-3 loop body of the Something-Something tree (STH/stage3.py:339-375 without AMP): the classifier
Linear and the local CNN learn (HIP forward and backward, PyTorch's SGD step on .grad); glancer and policy stay frozen.

``train_stage0_batch`` is the stage-0 loop body of the ActivityNet tree for the focuser's ResNet (ACT/main_dist.py:544-548,
pretrain_glancer=False, the branch without AMP): the local CNN and its ``fc`` learn on whole frames with BatchNorm on batch statistics
(HIP forward and backward).

``train_stage0_glancer_batch`` is the same loop body with pretrain_glancer=True: the glancer's MobileNetV2 and its classifier learn on
whole frames in train mode (``GFV.glancer_train_mode()``; HIP forward and backward).

``train_stage1_batch`` is the stage-1 loop body of the ActivityNet tree (ACT/main_dist.py:473-493 without AMP): the frozen glancer, one
random crop per frame through the local CNN on batch statistics, the GRU classifier, and the cross-entropy of every step
(``hip_ops.ce_steps``); the local CNN and the classifier learn.
"""
import torch
import torch.nn.functional as F

from . import hip_ops

__all__ = ["get_reward", "train_stage2_batch", "train_stage2_batch_fused", "train_stage2_batch_sth", "train_stage3_batch_sth",
           "train_stage0_batch", "train_stage0_glancer_batch", "train_stage1_batch"]


def get_reward(args, confidence, confidence_last, baseline):
    """main_dist.py:574-581: (reward, the confidence to carry to the next step)."""
    if args.reward == "prev":
        reward = confidence - confidence_last
    elif args.reward == "conf":
        reward = confidence
    elif args.reward == "random":
        reward = confidence - baseline
    else:
        raise NotImplementedError("reward %r" % (args.reward,))
    return reward, confidence


def train_stage2_batch(model, images, target, args):
    """One batch of stage-2 training.  images (B, T*3, H, W) normalised fp32 on the GPU, target (B,) int64 class indices.
    Glance, T roll-out steps with sampled actions, confidences -> rewards into model.focuser.memory.rewards, then model.focuser.update().
    Returns (predictions of every step stacked (T, B, C), the last step's cross-entropy)."""
    b = target.shape[0]
    t = args.num_segments
    input_prime = model.glancer_input(images)
    frames = images.view(b, t, 3, model.input_size, model.input_size)
    with torch.no_grad():
        global_feat_map, global_feat = model.glance(input_prime)
    confidence_last = 0
    local_results = []
    loss = None
    index = target.view(-1, 1)
    for step in range(t):
        output, pred, _, baseline_logits = model.one_step_act(frames[:, step], global_feat_map[:, step], global_feat[:, step],
                                                              restart_batch=step == 0, training=True)
        local_results.append(pred)
        loss = F.cross_entropy(output, target)
        confidence = torch.gather(F.softmax(output.detach(), 1), dim=1, index=index).view(1, -1)
        bsl_confidence = torch.gather(F.softmax(baseline_logits.detach(), 1), dim=1, index=index).view(1, -1)
        reward, confidence_last = get_reward(args, confidence, confidence_last, bsl_confidence)
        model.focuser.memory.rewards.append(reward)
    model.focuser.update()
    return torch.stack(local_results), loss


def train_stage2_batch_fused(model, images, target, args, uniforms=None):
    """train_stage2_batch with the T roll-out steps as one batched pass: glance, `model.rollout_act` (policy over all steps, one trunk pass
    over the B*T sampled crops, classifier scan and baseline branch), the rewards of all steps from `hip_ops.ppo_rewards` into
    model.focuser.memory.rewards as T (1, B) entries, then model.focuser.update().  uniforms (T, B) steers the sampling (None: torch.rand
    per step).  Same contract and return value: (predictions of every step stacked (T, B, C), the last step's cross-entropy)."""
    if args.reward not in hip_ops.REWARD_KINDS:
        raise NotImplementedError("reward %r" % (args.reward,))
    b = target.shape[0]
    t = args.num_segments
    input_prime = model.glancer_input(images)
    frames = images.view(b, t, 3, model.input_size, model.input_size)
    with torch.no_grad():
        global_feat_map, global_feat = model.glance(input_prime)
        logits, baseline = model._rollout_rows(frames, global_feat_map, global_feat, uniforms)        # rows b * T + t
        rewards, loss = hip_ops.ppo_rewards(logits, baseline, target, t, args.reward, want_ce_last=True)
        preds = logits.view(b, t, -1).transpose(0, 1).contiguous()
    model.focuser.memory.rewards.extend(rewards[s:s + 1] for s in range(t))
    model.focuser.update()
    return preds, loss[0]


def train_stage2_batch_sth(model, glancer_images, focuser_images, target, args, noise=None, baseline_actions=None):
    """One batch of stage-2 training of the Something-Something model (STH/stage2.py:233-270; `model.policy_train_mode()` first).
    glancer_images (B, Tg*3, g, g) already at the glance size, focuser_images (B, Tf*3, H, W), both normalised fp32 on the GPU, target (B,)
    int64.  Glance, `video_div` roll-out steps with actions sampled from the continuous policy, reward = confidence - the random
    baseline's confidence into model.focuser.memory.rewards, then model.focuser.update().  noise / baseline_actions: per step a (B, 2)
    tensor (standard normals of the sample / the baseline's action) or None for the reference's draws.
    Returns (the last step's prediction (B, C), its cross-entropy, the per-step rewards [(1, B)])."""
    b = target.shape[0]
    frames = focuser_images.view(b, args.num_segments_focuser, 3, focuser_images.shape[-2], focuser_images.shape[-1])
    with torch.no_grad():
        global_feat_map, global_feat_logit = model.glance(glancer_images)
    index = target.view(-1, 1)
    patches, rewards = None, []
    pred = loss = None
    for step in range(args.video_div):
        pred, baseline_logit, patches = model.action_stage2(frames, global_feat_map, global_feat_logit, step, args, prev_local_patch=patches,
                                                            training=True, noise=None if noise is None else noise[step],
                                                            baseline_action=None if baseline_actions is None else baseline_actions[step])
        loss = F.cross_entropy(pred, target)
        confidence = torch.gather(F.softmax(pred.detach(), 1), dim=1, index=index).view(1, -1)
        bsl_confidence = torch.gather(F.softmax(baseline_logit.detach(), 1), dim=1, index=index).view(1, -1)
        reward = confidence - bsl_confidence
        rewards.append(reward)
        model.focuser.memory.rewards.append(reward)
    model.focuser.update()
    return pred, loss, rewards


def train_stage3_batch_sth(model, glancer_images, focuser_images, target, args, optimizer, dropout_mask=None):
    """One batch of stage-3 training of the Something-Something model (STH/stage3.py:339-375, the branch without AMP;
    `model.stage3_train_mode()` first, optimizer = SGD(model.focuser.net.get_optim_policies() + [classifier]) as :189-193 builds it).
    glancer_images (B, Tg*3, g, g) already at the glance size, focuser_images (B, Tf*3, H, W), both normalised fp32 on the GPU, target (B,)
    int64.  zero_grad, glance without grad, action_stage3, cross-entropy, backward, optimizer.step().  dropout_mask (B*Tf, 2048) steers the
    dropout's draw (None: nn.Dropout's own).  Returns (the prediction (B, C), the loss)."""
    if args.video_div != 1:
        raise NotImplementedError("stage 3 is implemented for video_div == 1 only, as the reference asserts (STH/stage3.py:347)")
    b = target.shape[0]
    frames = focuser_images.view(b, args.num_segments_focuser, 3, focuser_images.shape[-2], focuser_images.shape[-1])
    optimizer.zero_grad()
    with torch.no_grad():
        global_feat_map, global_feat_logit = model.glance(glancer_images)
    pred, _ = model.action_stage3(frames, global_feat_map, global_feat_logit, 0, args, prev_local_patch=None, dropout_mask=dropout_mask)
    loss = F.cross_entropy(pred, target)
    loss.backward()
    optimizer.step()
    return pred.detach(), loss.detach()


def train_stage0_batch(model, images, target, args, optimizer):
    """One batch of stage-0 training of the focuser's ResNet (ACT/main_dist.py:544-548; `model.backbone_train_mode()` first, optimizer
    over model.focuser.net's parameters).  images (B, T*3, H, W) normalised fp32 on the GPU, target (B,) int64.  The frames go through the
    local CNN in train mode as one batch of B*T (BatchNorm statistics over all of them), the logits are averaged over T, then
    cross-entropy, backward, optimizer.step(); the gradients are zeroed first (main_dist.py:473).
    Returns (the prediction (B, C), the loss)."""
    b, tc, hh, ww = images.shape
    t = tc // 3
    optimizer.zero_grad()
    logits = model.focuser.net.forward_train(images.view(b * t, 3, hh, ww))
    pred = logits.view(b, t, -1).mean(1, keepdim=True).squeeze(1)
    loss = F.cross_entropy(pred, target)
    loss.backward()
    optimizer.step()
    return pred.detach(), loss.detach()


def train_stage0_glancer_batch(model, images, target, args, optimizer, dropout_mask=None):
    """One batch of stage-0 training of the glancer's MobileNetV2 (ACT/main_dist.py:544-548 with pretrain_glancer=true;
    `model.glancer_train_mode()` first, optimizer over model.glancer.net's parameters).  images (B, T*3, H, W) normalised fp32 on the GPU,
    target (B,) int64.  The frames go through the MobileNetV2 in train mode as one batch of B*T (BatchNorm statistics over all of them,
    Dropout(0.2) in front of the Linear), the logits are averaged over T, then cross-entropy, backward, optimizer.step(); the gradients
    are zeroed first (main_dist.py:473).  dropout_mask (B*T, 1280) gives the dropout's multipliers (None: drawn from torch's device
    generator).  Returns (the prediction (B, C), the loss), detached."""
    b, tc, hh, ww = images.shape
    t = tc // 3
    optimizer.zero_grad()
    logits = model.glancer.net.forward_train(images.view(b * t, 3, hh, ww), dropout_mask=dropout_mask)
    pred = logits.view(b, t, -1).mean(1, keepdim=True).squeeze(1)
    loss = F.cross_entropy(pred, target)
    loss.backward()
    optimizer.step()
    return pred.detach(), loss.detach()


def train_stage1_batch(model, images, target, args, optimizer, crop_actions=None, dropout_mask=None):
    """One batch of stage-1 training (ACT/main_dist.py:473-493; `model.stage1_train_mode()` first, optimizer = main_dist.py:172-177's SGD
    over model.focuser.parameters() and model.classifier.parameters(); focuser.net.fc takes no part and gets no gradient).  images
    (B, T*3, H, W) normalised fp32 on the GPU, target (B,) int64.  zero_grad, `model.glancer_input`, the stage-1 form of the forward in
    train mode (frozen glancer, one random crop per frame, the local CNN over the B*T patches as one batch on batch statistics, the GRU
    classifier with dropout), the mean cross-entropy of all B*T steps against the clip's label (`hip_ops.ce_steps`: main_dist.py:479's
    expanded target, not materialised), backward, optimizer.step().
    The call form: the reference's non-AMP call (main_dist.py:486) omits `training=` while gfv_net.py:146 reads kwargs["training"], so
    that branch cannot run as written; mirrored is the AMP branch's call (:477, training=True) with the loss of :479, without autocast
    and the scaler.
    crop_actions (B*T, 2) / dropout_mask (B, T, hidden) steer the crops (the gather's actions) and the dropout's multipliers (None: drawn
    as the reference draws them / from torch's device generator).  Returns (the last step's prediction (B, C), the loss), detached."""
    t = images.shape[1] // 3
    optimizer.zero_grad()
    input_prime = model.glancer_input(images)
    output, pred = model(input=images, scan=input_prime, backbone_pred=False, one_step=False, training=True, crop_actions=crop_actions,
                         dropout_mask=dropout_mask)
    loss = hip_ops.CeStepsFn.apply(output, target, t)
    loss.backward()
    optimizer.step()
    return pred.detach(), loss.detach()[0]
