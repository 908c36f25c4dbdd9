"""Host-side checks of stage-3 training of the Something-Something local CNN (no GPU): TSN.get_optim_policies against the parameter names
the reference's get_optim_policies returned (tests/golden/g20_sth_stage3.npz, tools/gen_golden_stage3_sth.py), the shapes the gradients
take, and the partial-BN rule of TSN.train()."""
import pytest
import torch

from tests.helpers import golden, manifest
from tests.test_state_dict_compat import sth_args


def _model(partial_bn):
    from adafocus_amd.gfv_net_sth import GFV
    a = sth_args()
    a.partial_bn = partial_bn
    m = GFV(a)
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])      # STH/stage3.py:87
    return m


@pytest.mark.parametrize("pbn", [0, 1])
def test_optim_policies_match_the_reference(pbn):
    """Group by group: the reference's names in the reference's order, its group names and lr_mult / decay_mult; every parameter has the
    shape of the reference's state dict, which is the shape its .grad takes."""
    g = golden("g20_sth_stage3")
    m = _model(bool(pbn))
    names = {id(v): k for k, v in m.state_dict(keep_vars=True).items()}
    policies = m.focuser.net.get_optim_policies()
    assert [p["name"] for p in policies] == g["group_names"].tolist()
    assert [[p["lr_mult"], p["decay_mult"]] for p in policies] == g["group_mults"].tolist()
    shapes = manifest()["STH"]
    total = 0
    for i, p in enumerate(policies):
        got = [names[id(q)] for q in p["params"]]
        assert got == g["groups_pbn%d_%d" % (pbn, i)].tolist(), p["name"]
        for q, n in zip(p["params"], got):
            assert tuple(q.shape) == shapes[n] and q.requires_grad, n
        total += len(got)
    trunk = [k for k in shapes if k.startswith("focuser.net.") and k.endswith((".weight", ".bias"))]
    assert total == (len(trunk) if not pbn else 53 + 2)          # every conv weight + every BatchNorm pair, or the first pair only
    # the construction of STH/stage3.py:189-193 runs as it is written there
    opt = torch.optim.SGD(policies + [{"params": m.classifier.parameters()}], lr=0, momentum=0.9, weight_decay=5e-4)
    assert len(opt.param_groups) == 6


def test_partial_bn_freezes_later_batchnorms_in_train_mode():
    """STH/models/tsn.py:146-162: train() with partial BN takes every BatchNorm of the base model but the first out of training."""
    m = _model(True)
    net = m.focuser.net
    bns = [q for q in net.base_model.modules() if isinstance(q, torch.nn.BatchNorm2d)]
    assert all(b.weight.requires_grad for b in bns)
    m.train()
    assert bns[0].weight.requires_grad and bns[0].bias.requires_grad
    assert not any(b.weight.requires_grad or b.bias.requires_grad for b in bns[1:])
    m2 = _model(False)
    m2.train()
    assert all(b.weight.requires_grad for b in m2.focuser.net.base_model.modules() if isinstance(b, torch.nn.BatchNorm2d))


def test_stage3_train_mode_sets_the_reference_modes():
    m = _model(False)
    assert not m.focuser.net.base_model.trainable
    m.stage3_train_mode()
    assert m.training and m.dropout.training and not m.glancer.training and not m.focuser.training
    assert not m.focuser.policy.policy.training and not m.focuser.policy.policy_old.training
    assert m.focuser.net.base_model.trainable
    m.stage3_train_mode(train_local=False)
    assert not m.focuser.net.base_model.trainable
