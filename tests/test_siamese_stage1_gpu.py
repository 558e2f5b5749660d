"""GPU: FD-GAN stage I — `reid.trainers.SiameseTrainer` on `SiameseNet.forward_loss` (both trunk passes, the fused verification head
of csrc/verif_head.hip, nn.CrossEntropyLoss() and `accuracy` as one tape program), FD/reid/trainers.py:62-73 under FD/baseline.py's
optimizer (SGD, momentum 0.9, weight decay 5e-4, two groups with `lr_mult`).

The step host model is composed here from pieces oracle/ already ties to the reference: O.OSiameseNet(O.OReidResNet(18,
cut_at_pooling=True), O.OEltwiseSubEmbed(...)), F.cross_entropy, the argmax count and torch's SGD.  Shape: 4 pairs of 64x32 crops.

A conditioned start, as in tests/test_hardmix_gpu.py: the last BatchNorm scale of every residual block starts in U(0.02, 0.04), so
that three train-mode-BatchNorm steps at a batch of 4 are not chaotic inside the host model itself; the classifier starts at
normal(0, 0.05) (with the reference's 0.001 the two logits of a row differ by roundings and `prec` would be decided by them).  The
host fixture runs the trajectory in float32 and in float64 and asserts, as a test-construction check, that its own float32 losses lie
within a quarter of the 1e-3 bound of the float64 ones and that no row's two logits are closer than 1e-3 on any step.  The bounds
are tests/test_hardmix_gpu.py's: 1e-3 on a loss, 2e-3 (relative L2) on the parameters and on the running statistics after three steps.

What pins the two-pass trunk gradient is the LOSS of steps 2 and 3, not the parameter bound: at this learning rate the trunk's
weights move by 4e-4 of the sampled parameters' norm in three steps, so a wrong trunk gradient stays inside 2e-3 there (that bound
catches a wrong head gradient, a missed weight decay or momentum and stale statistics).  The losses feel it: the fixture also runs the
host model with the trunk gradient halved and without any update, and asserts that either moves the losses of steps 2 and 3 by more
than ten times their bound.

The host trajectory is computed once (module-scoped) and shared, unchanged, by the tests that need it."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_torch as O

pytestmark = pytest.mark.gpu

SEED = 11
B, STEPS = 4, 3
LR, MOMENTUM, WD = 0.01, 0.9, 5e-4
LOSS_TOL, STATE_TOL = 1e-3, 2e-3        # tests/test_hardmix_gpu.py's bounds
LOGIT_MARGIN = 1e-3


def _groups(net):
    # FD/baseline.py:126-130
    return [{'params': list(net.base_model.parameters()), 'lr_mult': 0.1, 'lr': LR * 0.1},
            {'params': list(net.embed_model.parameters()), 'lr_mult': 1.0, 'lr': LR}]


def _host_net(dtype=torch.float32):
    torch.manual_seed(SEED)
    base = O.OReidResNet(18, cut_at_pooling=True)
    embed = O.OEltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=512, num_classes=2)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for n, m in base.named_modules():
            if n.endswith("bn2"):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.02 + 0.02)
        embed.classifier.weight.copy_(torch.randn(embed.classifier.weight.shape, generator=g) * 0.05)
    return O.OSiameseNet(base, embed).to(dtype).train()


def _inputs():
    g = torch.Generator().manual_seed(SEED + 2)
    items = []
    for i in range(STEPS):
        x1, x2 = O.synth_images(B, 64, 32, seed=SEED + 10 + i), O.synth_images(B, 64, 32, seed=SEED + 20 + i)
        pids1 = torch.randint(0, 3, (B,), generator=g)
        pids2 = torch.where(torch.rand(B, generator=g) < 0.5, pids1, pids1 + 1)
        items.append((x1, x2, pids1, pids2))
    return items


def _host_run(dtype, start=None, update=True, trunk_grad_scale=None):
    net = _host_net(dtype)
    if start is not None:
        net.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in start.items()})
    first = copy.deepcopy(net.state_dict())
    opt = torch.optim.SGD(_groups(net), LR, momentum=MOMENTUM, weight_decay=WD)
    losses, precs, margins = [], [], []
    for x1, x2, p1, p2 in _inputs():
        y = (p1 == p2).long()
        _, _, logits = net(x1.to(dtype), x2.to(dtype))
        loss = F.cross_entropy(logits, y)
        precs.append(float((logits.argmax(1) == y).float().mean()))
        margins.append(float((logits[:, 0] - logits[:, 1]).detach().abs().min()))
        opt.zero_grad()
        loss.backward()
        if trunk_grad_scale is not None:
            for p in net.base_model.parameters():
                if p.grad is not None:
                    p.grad.mul_(trunk_grad_scale)
        if update:
            opt.step()
        losses.append(loss.item())
    return dict(start=first, losses=losses, precs=precs, margins=margins,
                params={n: p.detach().clone() for n, p in net.named_parameters()},
                buffers={n: b.detach().clone() for n, b in net.named_buffers()})


@pytest.fixture(scope="module")
def host():
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    h32 = _host_run(torch.float32)
    h64 = _host_run(torch.float64, h32["start"])
    h32["losses64"] = h64["losses"]
    h32["precs64"] = h64["precs"]
    h32["losses_frozen"] = _host_run(torch.float32, h32["start"], update=False)["losses"]      # the weights never move
    h32["losses_half_trunk"] = _host_run(torch.float32, h32["start"], trunk_grad_scale=0.5)["losses"]
    return h32


def test_host_model_is_conditioned(host):
    """a test-construction check: the host model's own float32 run stays within a quarter of the loss bound of its float64 run, both
    count the same rows correct, and no row's logits are within 1e-3 of a tie"""
    for i in range(STEPS):
        print("step %d host loss %.6f float64 %.6f prec %.2f margin %.3e" % (i, host["losses"][i], host["losses64"][i], host["precs"][i],
                                                                             host["margins"][i]))
        assert abs(host["losses"][i] - host["losses64"][i]) <= 0.25 * LOSS_TOL * abs(host["losses64"][i])
        assert host["precs"][i] == host["precs64"][i] and host["margins"][i] >= LOGIT_MARGIN
    # a step that saw stale weights is far outside the bound: without the optimizer's updates the later losses are elsewhere
    for i in (1, 2):
        for what in ("losses_frozen", "losses_half_trunk"):
            gap = abs(host[what][i] - host["losses"][i]) / abs(host["losses"][i])
            print("step %d %s %.6f: %.3e away" % (i, what, host[what][i], gap))
            assert gap > 10 * LOSS_TOL, "step %d: %s moves the loss by %.3e only" % (i, what, gap)


def _gpu_parts(dev, host, optimizer="torch", wrap=None, criterion=None, **kw):
    import reid.models as RM
    from reid.models.embedding import EltwiseSubEmbed
    from reid.models.multi_branch import SiameseNet
    from reid.trainers import SiameseTrainer
    from rg_hip import optim as roptim
    base = RM.create('resnet18', pretrained=False, cut_at_pooling=True)
    embed = EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=512, num_classes=2)
    net = SiameseNet(base, embed)
    net.load_state_dict(host["start"])
    net = net.to(dev).train()
    cls = torch.optim.SGD if optimizer == "torch" else roptim.SGD
    opt = cls(_groups(net), LR, momentum=MOMENTUM, weight_decay=WD)
    model = net if wrap is None else wrap(net)
    trainer = SiameseTrainer(model, nn.CrossEntropyLoss() if criterion is None else criterion, **kw)
    return net, opt, trainer


def _rel_l2(got, ref, names):
    num = sum(float((got[n].detach().double().cpu() - ref[n].double()).pow(2).sum()) for n in names)
    den = sum(float(ref[n].double().pow(2).sum()) for n in names)
    return (num / den) ** 0.5


def _three_steps(dev, host, trainer):
    out = []
    for x1, x2, p1, p2 in _inputs():
        inputs, targets = trainer._parse_data(((x1, None, p1, None), (x2, None, p2, None)))
        out.append(trainer.step(inputs[0], inputs[1], targets, trainer._opt))
    return out


def _check_trajectory(net, host, steps, what):
    for i, (loss, prec) in enumerate(steps):
        assert loss.dim() == 0 and prec.dim() == 0 and loss.is_cuda and not loss.requires_grad
        print("%s step %d loss %.6f host %.6f prec %.2f" % (what, i, loss.item(), host["losses"][i], prec.item()))
        assert abs(loss.item() - host["losses"][i]) <= LOSS_TOL * abs(host["losses"][i]), (what, i, loss.item(), host["losses"][i])
        assert prec.item() == host["precs"][i], (what, i, prec.item(), host["precs"][i])
    g = torch.Generator().manual_seed(3)
    names = list(host["params"])
    sample = [names[int(j)] for j in torch.randperm(len(names), generator=g)[:24]] + [n for n in names if n.startswith("embed_model")]
    err = _rel_l2(dict(net.named_parameters()), host["params"], sample)
    print("%s parameters after %d steps: rel L2 %.3e" % (what, STEPS, err))
    assert err <= STATE_TOL, "%s parameters after three steps: rel L2 %.3e" % (what, err)
    state = net.state_dict()                             # (the counters are kept on the host and written when the state is read)
    stats = [n for n in host["buffers"] if n.endswith("running_mean") or n.endswith("running_var")]
    err = _rel_l2(state, host["buffers"], stats)
    print("%s running statistics after %d steps: rel L2 %.3e" % (what, STEPS, err))
    assert err <= STATE_TOL, "%s running statistics: rel L2 %.3e" % (what, err)
    for n, b in host["buffers"].items():
        if n.endswith("num_batches_tracked"):
            want = STEPS if n.startswith("embed_model") else 2 * STEPS          # the trunk sees two batches per step
            assert int(state[n]) == want == int(b), (n, int(state[n]), int(b))


@pytest.mark.parametrize("optimizer", ["torch", "rg_hip"])
def test_three_steps_against_the_host_model(dev, host, optimizer):
    net, opt, trainer = _gpu_parts(dev, host, optimizer)
    trainer._opt = opt
    assert trainer._siamese() is net
    _check_trajectory(net, host, _three_steps(dev, host, trainer), "fused/" + optimizer)
    assert net.training


def test_composed_path_agrees(dev, host):
    """`fused_head=False` runs the reference's three lines on the composed layers: the same trajectory within the same bounds, and
    the three steps of the two paths from the same start within the loss bound of each other"""
    net, opt, trainer = _gpu_parts(dev, host, fused_head=False)
    trainer._opt = opt
    assert trainer._siamese() is None
    steps = _three_steps(dev, host, trainer)
    _check_trajectory(net, host, steps, "composed")
    net2, opt2, trainer2 = _gpu_parts(dev, host)
    trainer2._opt = opt2
    for i, ((loss, prec), (closs, cprec)) in enumerate(zip(_three_steps(dev, host, trainer2), steps)):      # steps 2 and 3 carry the gradients
        assert abs(loss.item() - closs.item()) <= LOSS_TOL * abs(closs.item()) and prec.item() == cprec.item(), (i, loss.item(), closs.item())


def test_train_is_three_step_calls_and_prints_the_reference_line(dev, host, capsys):
    items = [((x1, ["a"] * B, p1, torch.zeros(B)), (x2, ["b"] * B, p2, torch.zeros(B))) for x1, x2, p1, p2 in _inputs()]
    net1, opt1, tr1 = _gpu_parts(dev, host)
    capsys.readouterr()
    tr1.train(0, items, opt1, print_freq=1)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch: [0][")]
    assert len(lines) == STEPS and lines[-1].startswith("Epoch: [0][3/3]\tTime ")
    assert all("\tLoss " in l and "\tPrec " in l and l.endswith("%)\t") for l in lines), lines
    net2, opt2, tr2 = _gpu_parts(dev, host)
    tr2._opt = opt2
    steps = _three_steps(dev, host, tr2)
    sa, sb = net1.state_dict(), net2.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), "train() and three step() calls differ"
    for l, (loss, prec) in zip(lines, steps):
        assert float(l.split("Loss")[1].split()[0]) == float("%.3f" % loss.item())
        assert l.split("Prec")[1].split()[0] == "{:.2%}".format(prec.item())
    # the deferred meters: one print interval of three steps gives the same averages
    net3, opt3, tr3 = _gpu_parts(dev, host)
    capsys.readouterr()
    tr3.train(1, items, opt3, print_freq=STEPS)
    out3 = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch: [1][")]
    assert len(out3) == 1 and out3[0].split("Loss")[1] == lines[-1].split("Loss")[1]


def test_wrapped_model_label_smoothing_and_eval_trunk(dev, host):
    from rg_hip import parallel
    from rg_hip.resnet_trunk import bn_all_eval
    x1, x2, p1, p2 = _inputs()[0]
    ref = None
    for wrap in (None, nn.DataParallel, parallel.DataParallel):
        net, opt, trainer = _gpu_parts(dev, host, wrap=(lambda n: wrap(n)) if wrap is not None else None)
        assert trainer._siamese() is net
        inputs, targets = trainer._parse_data(((x1, None, p1, None), (x2, None, p2, None)))
        loss, prec = trainer.step(inputs[0], inputs[1], targets, opt)
        if ref is None:
            ref = (loss.clone(), net.state_dict())
        else:
            assert torch.equal(loss, ref[0]) and all(torch.equal(v, ref[1][k]) for k, v in net.state_dict().items())
    # a criterion the head does not fuse takes the composed layers
    net, opt, trainer = _gpu_parts(dev, host, criterion=nn.CrossEntropyLoss(label_smoothing=0.1))
    assert trainer._siamese() is None
    inputs, targets = trainer._parse_data(((x1, None, p1, None), (x2, None, p2, None)))
    loss, prec = trainer.step(inputs[0], inputs[1], targets, opt)
    assert bool(torch.isfinite(loss)) and abs(loss.item() - ref[0].item()) > 1e-4
    # every BatchNorm of the trunk in eval mode: one batched pass, no statistic of the trunk moves, the head's do
    net, opt, trainer = _gpu_parts(dev, host)
    net.base_model.eval()
    assert bn_all_eval(net.base_model)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    calls = []
    tf = net.base_model.tf
    net.base_model.tf = lambda tape, x: calls.append(x.shape[0]) or tf(tape, x)
    f1, f2, logits, loss, prec = net.forward_loss(inputs[0], inputs[1], targets)
    assert calls == [2 * B] and f1.shape == (B, 512) and logits.shape == (B, 2)
    loss.backward()
    after = net.state_dict()
    for k in before:
        moved = not torch.equal(before[k], after[k])
        if k.startswith("base_model") and ("running_" in k or "num_batches" in k):
            assert not moved, k
        if k.startswith("embed_model.bn.running_") or k == "embed_model.bn.num_batches_tracked":
            assert moved, k
    missing = [n for n, p in net.named_parameters() if p.grad is None and ".fc." not in n]      # the trunk's `fc` is never run
    assert not missing, missing
    # the module call is what it was
    o1, o2, lg = net(inputs[0], inputs[1])
    assert lg.shape == (B, 2)
