"""Stage-2 training loop body (ACT/main_dist.py:494-518, 574-581): the PPO roll-out over T focus steps and the policy update.

    model.policy_train_mode()                 # in place of the reference's model.train_mode(args) at train_stage == 2
    for images, target in loader:
        preds, loss = train_stage2_batch(model, images.cuda(), target[:, 0].cuda(), args)

Both CNNs and the classifier stay frozen and run on the HIP path; only ``focuser.policy.policy`` learns (``PPO.update``: HIP forward and
backward, PyTorch's Adam step).
"""
import torch
import torch.nn.functional as F

__all__ = ["get_reward", "train_stage2_batch"]


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
