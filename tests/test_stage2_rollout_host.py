"""The batched stage-2 roll-out without a device: the two new C-ABI exports with their prototypes, and the fused loop body's export."""
import ctypes
import os
import re

from adafocus_amd import _lib, hip_ops, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, IP = ctypes.c_void_p, ctypes.c_int
PROTOTYPES = {
    # h, logits, ld, steps, batch, n_actions, uniforms, table_yx, action_out, logprob_out, coords_out, stream
    "adaf_ppo_sample_actions_f32": [VP, VP, IP, IP, IP, IP, VP, VP, VP, VP, VP, VP],
    # h, logits, base_logits, target, steps, batch, classes, kind, rewards_out, conf_out, ce_last_out, stream
    "adaf_ppo_rewards_f32": [VP, VP, VP, VP, IP, IP, IP, IP, VP, VP, VP, VP],
}


def test_new_exports_declared_everywhere():
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name, argtypes in PROTOTYPES.items():
        assert name in _lib.SYMBOLS
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(argtypes), name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is ctypes.c_int
    assert lib.adaf_version() == 303
    # neither call has a workspace: no query was added for them
    assert not [s for s in _lib.SYMBOLS if re.match(r"adaf_ppo_(sample_actions|rewards)\w*workspace", s)]


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load_library()
    assert lib.adaf_ppo_sample_actions_f32(None, None, 0, 1, 1, 4, None, None, None, None, None, None) == -1
    assert lib.adaf_ppo_rewards_f32(None, None, None, None, 1, 1, 4, 0, None, None, None, None) == -1


def test_reward_kinds_match_the_header():
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    for name, num in hip_ops.REWARD_KINDS.items():
        assert re.search(r"ADAF_REWARD_%s = %d\b" % (name.upper(), num), header), name


def test_fused_body_is_exported():
    assert "train_stage2_batch_fused" in train.__all__ and callable(train.train_stage2_batch_fused)
    assert "train_stage2_batch" in train.__all__
