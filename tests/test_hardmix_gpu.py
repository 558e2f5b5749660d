"""GPU: the hard-mix ReID step (`ClusterContrastWithGANTrainer.hard_mix_step`, CC/clustercontrast/trainers.py:65-72, 96-98), the
loop on it (`train` with a ClusterMemory_Gradient, :34-127) and the warm-up loop `train_reid` (trainers_b.py:1087-1138).

The step host model is composed here from pieces oracle/ already ties to the reference: O.OCCResNet(50), D.OAEGenerator
(forward_enc / forward_dec), D.o_hard_mix, D.o_my_transform, O.OClusterMemoryGradient and torch's Adam, one group per tensor.
Shape: 8 crops of 64x32 in identity groups of 2 (4 synthesised images), 6 clusters, GAN inputs of 64x32, model="AE" / model_gen="AE".

The mix selections are discrete (an argmin and an argmax per identity), so the host model reports by how much each one wins and the
test asserts a margin of 1e-3 on every step: below it a rounding difference could pick another sample and the two sides would
not compute the same step.  SEED was chosen so that this holds on the CPU.

A conditioned start.  Three consecutive steps of a RAW randomly initialised train-mode-BatchNorm ResNet-50 at this batch are
chaotic inside the host model itself: at the script's Adam (lr 3.5e-4, weight decay 5e-4) its own float32 CPU losses of steps
1 and 2 move by 2 % and 4 % when only the thread count changes (8 -> 1 threads: 2.3325 -> 2.2827, 2.7398 -> 2.5962; 4e-3 ..
4e-2 from a float64 run of the same model), and the selection margins with them, so no 1e-3 comparison of steps 1 and 2 could
hold between ANY two float32 implementations.  The initial weights are this test's to choose, so the last BatchNorm scale of
every bottleneck starts in U(0.02, 0.04) (the usual small-residual start).  Measured on the CPU with that start: the float32
host losses (2.47823, 2.86898, 3.05009) are within 4e-6 of the float64 run on all three steps at 1, 3 and 8 threads, the margins
(4.2e-3, 3.8e-3, 1.5e-2) do not depend on the thread count, and the loss still moves by 0.2 .. 0.4 from step to step under the
script's learning rate, so a step that saw stale weights or statistics is far outside 1e-3.

The host trajectory is computed once (module-scoped) and shared, unchanged, by the tests that need it."""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_dualgan as D
from oracle import ref_torch as O
from tests.test_modules_gpu import _check_l2
from tests.test_paths_gpu import _Loader, _cc_parts

pytestmark = pytest.mark.gpu

SEED = 5
B, GROUP, K, STEPS = 8, 2, 6, 3
LAMBDA_FUS = 0.8
MARGIN = 1e-3


def _adam(net, cls):
    # one Adam group per tensor, as the reference's script builds it (examples/cluster_contrast_gan_train_usl_infomap.py:281-284)
    return cls([{"params": [p]} for p in net.parameters() if p.requires_grad], lr=3.5e-4, weight_decay=5e-4)


def _inputs():
    """per step: (crops [B, 3, 64, 32], labels [B] in identity groups of GROUP, GAN source images [B, 3, 64, 32])"""
    g = torch.Generator().manual_seed(SEED + 100)
    items = []
    for i in range(STEPS):
        x = O.synth_images(B, 64, 32, seed=SEED + 10 + i)
        labels = torch.randperm(K, generator=g)[:B // GROUP].repeat_interleave(GROUP)
        xs = D.synth_dualgan_inputs(B, 64, 32, seed=SEED + 20 + i)['Xs']
        items.append((x, labels, xs))
    return items


def _host_parts():
    from tests.golden import cases_dualgan as C
    torch.manual_seed(SEED)
    oenc = O.OCCResNet(50, pooling_type="gem").train()
    og, _ = C.aegen_case()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():                                # a conditioned start: see the module docstring
        for n, m in oenc.named_modules():
            if n.endswith("bn3"):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.02 + 0.02)
    clusters = torch.randn(K, oenc.num_features, generator=g)
    return oenc, og, clusters


def _mix_margins(reid_f, group):
    """by how much the argmin / argmax of D.o_hard_mix win (its similarities restated): (in-identity margin, other-identity margin),
    each the smallest over the identities; an identity with a single candidate has an infinite margin"""
    fdim = reid_f.shape[1]
    anchor = F.normalize(torch.mean(reid_f.reshape(-1, group, fdim), dim=1))
    sim = torch.exp(anchor @ F.normalize(reid_f).t())
    id_mask = torch.eye(anchor.shape[0]).repeat_interleave(group, dim=1)
    lo = torch.sort(id_mask * sim + (1 - id_mask) * torch.max(sim), dim=1).values
    hi = torch.sort((1 - id_mask) * sim, dim=1, descending=True).values
    inf = torch.tensor(float("inf"))
    return (float((lo[:, 1] - lo[:, 0]).min()) if lo.shape[1] > 1 else inf, float((hi[:, 0] - hi[:, 1]).min()) if hi.shape[1] > 1 else inf)


def _host_step(oenc, og, om, oopt, x, labels, xs, ex=True):
    """one step of the reference's loop on the oracle pieces -> (loss, f_ex, margins)"""
    f_out = oenc(x)[0]
    f_ex, margins = None, None
    if ex:
        with torch.no_grad():
            margins = _mix_margins(f_out.detach(), GROUP)
            img = og.forward_dec(D.o_hard_mix(og.forward_enc(xs), f_out.detach(), GROUP, LAMBDA_FUS))
            oenc.eval()
            f_ex = oenc(D.o_my_transform(img))
            oenc.train()
    loss = om.forward(f_out, labels, f_ex)
    oopt.zero_grad()
    loss.backward()
    oopt.step()
    return loss.item(), f_ex, margins


@pytest.fixture(scope="module")
def host():
    """the host trajectory of three hard-mix steps and of three plain warm-up steps, from the same start"""
    oenc, og, clusters = _host_parts()
    start = copy.deepcopy(oenc.state_dict())
    gen_state = copy.deepcopy(og.state_dict())
    items = _inputs()
    om = O.OClusterMemoryGradient(temp=0.05)
    om.set_clusters(clusters, 0.1)
    oopt = _adam(oenc, torch.optim.Adam)
    steps = [_host_step(oenc, og, om, oopt, *it) for it in items]
    mix = dict(losses=[s[0] for s in steps], f_ex=[s[1] for s in steps], margins=[s[2] for s in steps],
               params={n: p.detach().clone() for n, p in oenc.named_parameters()},
               buffers={n: b.detach().clone() for n, b in oenc.named_buffers()})
    oenc2 = O.OCCResNet(50, pooling_type="gem").train()
    oenc2.load_state_dict(start)
    om2 = O.OClusterMemoryGradient(temp=0.05)
    om2.set_clusters(clusters, 0.1)
    oopt2 = _adam(oenc2, torch.optim.Adam)
    warm = [_host_step(oenc2, og, om2, oopt2, *it, ex=False)[0] for it in items]
    return dict(start=start, gen=gen_state, clusters=clusters, items=items, mix=mix, warm=warm)


def _gpu_parts(dev, host):
    """encoder, GAN, learnable memory, optimizer and trainer on the host model's start"""
    import clustercontrast.models as M
    from clustercontrast.models.cm import ClusterMemory_Gradient
    from clustercontrast.trainers import ClusterContrastWithGANTrainer
    from dual_gan.models.models import create_model
    from rg_hip import optim as roptim
    from tests.test_dualgan_gpu import _gan_opt
    enc = M.create('resnet50', pretrained=False, pooling_type="gem")
    enc.load_state_dict(host["start"])
    enc = enc.to(dev).train()
    gan = create_model(_gan_opt(model="AE", model_gen="AE", lambda_fus=LAMBDA_FUS))
    gan.net_G.module.load_state_dict(host["gen"])
    mem = ClusterMemory_Gradient(enc.num_features, K, temp=0.05)
    mem.set_clusters(host["clusters"].to(dev), 0.1)
    opt = _adam(enc, roptim.Adam)
    trainer = ClusterContrastWithGANTrainer(enc, GAN=gan, memory=mem, opt=argparse.Namespace(num_instances=GROUP, cl_temp=0.05))
    trainer.sync_every_step = True
    return enc, gan, mem, opt, trainer


def _loader(host):
    items = []
    for x, labels, xs in host["items"]:
        reid = (x, ["f"] * B, labels, torch.zeros(B, dtype=torch.long), torch.arange(B))
        items.append([reid, {"Xs": xs, "Xs_path": ["a"] * B, "gt_label": torch.zeros(B)}])
    return _Loader(items)


def _printed_losses(out):
    return [float(l.split("Loss")[1].split()[0]) for l in out.splitlines() if l.startswith("Epoch: [")]


def test_selection_margins_of_the_host_model(host):
    """a test-construction check: every argmin / argmax of the mix wins by at least 1e-3 on every step"""
    for i, (lo, hi) in enumerate(host["mix"]["margins"]):
        print("step %d margins: in-identity %.3e other-identity %.3e" % (i, lo, hi))
        assert lo >= MARGIN and hi >= MARGIN, "step %d: selection margins %.3e / %.3e below %.0e — choose another SEED" % (i, lo, hi, MARGIN)


def test_three_hard_mix_steps(dev, host):
    enc, gan, mem, opt, trainer = _gpu_parts(dev, host)
    ref = host["mix"]
    gan_before = {n: p.detach().clone() for n, p in gan.net_G.named_parameters()}
    clusters_before = mem.trainable_clusters.detach().clone()
    seen = []
    embed = trainer._embed_hard_mix
    trainer._embed_hard_mix = lambda f, g: seen.append(embed(f, g)) or seen[-1]
    for i, (x, labels, xs) in enumerate(host["items"]):
        gan.set_input({"Xs": xs})
        loss = trainer.hard_mix_step(x.to(dev), labels.to(dev), opt).item()          # group_size defaults to opt.num_instances
        print("step %d loss %.6f host %.6f" % (i, loss, ref["losses"][i]))
        assert abs(loss - ref["losses"][i]) <= 1e-3 * abs(ref["losses"][i]), "step %d loss %r vs %r" % (i, loss, ref["losses"][i])
        assert seen[i].shape == (B // GROUP, enc.num_features) and not seen[i].requires_grad
        _check_l2(seen[i], ref["f_ex"][i], 1e-3, "f_ex of step %d" % i)
    got = dict(enc.named_parameters())
    num = sum(float((got[n].detach().double().cpu() - p.double()).pow(2).sum()) for n, p in ref["params"].items())
    den = sum(float(p.double().pow(2).sum()) for p in ref["params"].values())
    print("encoder parameters after %d steps: rel L2 %.3e" % (STEPS, (num / den) ** 0.5))
    assert (num / den) ** 0.5 <= 2e-3, "encoder parameters after three steps: rel L2 %.3e" % (num / den) ** 0.5
    # nothing in this loop updates the centroids, as in the reference
    assert torch.equal(mem.trainable_clusters.detach(), clusters_before)
    # the eval pass moved no statistic: the buffers are those of three train-mode forwards (the host model's, whose eval pass is
    # torch's), and every counter stands at three
    state = enc.state_dict()                             # (the counters are kept on the host and written when the state is read)
    for n in ref["buffers"]:
        if n.endswith("num_batches_tracked"):
            assert int(state[n]) == STEPS == int(ref["buffers"][n]), (n, int(state[n]))
    stats = [n for n in ref["buffers"] if n.endswith("running_mean") or n.endswith("running_var")]
    got = state
    num = sum(float((got[n].double().cpu() - ref["buffers"][n].double()).pow(2).sum()) for n in stats)
    den = sum(float(ref["buffers"][n].double().pow(2).sum()) for n in stats)
    print("encoder running statistics after %d steps: rel L2 %.3e" % (STEPS, (num / den) ** 0.5))
    # a function of the parameters of steps 0..2: the parameters' own bound; an eval pass that updated them (momentum 0.1) is 1e-1 away
    assert (num / den) ** 0.5 <= 2e-3, "encoder running statistics: rel L2 %.3e" % (num / den) ** 0.5
    assert enc.training and all(m.training for m in enc.modules())
    for n, p in gan.net_G.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), gan_before[n]), "the GAN's %s moved or has a gradient" % n


def test_eval_pass_sees_the_current_weights_and_statistics(dev, host):
    """the eval pass after an optimizer step, an evaluation (which folds the BatchNorms for those weights) and a train-mode pass
    (which moves the running statistics and not the weights): f_ex is what a freshly built encoder with the same state gives,
    no buffer moves in the eval pass, and the encoder comes back in train mode"""
    import clustercontrast.models as M
    from clustercontrast.utils.data.diff_augs import my_transform
    enc, gan, mem, opt, trainer = _gpu_parts(dev, host)
    x, labels, xs = host["items"][0]
    gan.set_input({"Xs": xs})
    trainer.hard_mix_step(x.to(dev), labels.to(dev), opt)
    with torch.no_grad():
        enc.eval()
        enc(O.synth_images(2, 64, 32, seed=5).to(dev))
        enc.train()
    names = [n for n, _ in enc.named_buffers()]          # running statistics and counters, read through state_dict()
    before = {n: b.clone() for n, b in enc.state_dict().items() if n in names}
    f_out = enc(x.to(dev))[0].detach()
    stats = {n: b.clone() for n, b in enc.state_dict().items() if n in names}
    assert all(not torch.equal(stats[n], before[n]) for n in stats)
    f_ex = trainer._embed_hard_mix(f_out, GROUP)
    for n, b in enc.state_dict().items():
        assert n not in stats or torch.equal(b, stats[n]), "the eval pass moved " + n
    assert enc.training and all(m.training for m in enc.modules())
    fresh = M.create('resnet50', pretrained=False, pooling_type="gem")
    fresh.load_state_dict(enc.state_dict())
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        ref = fresh(my_transform(gan.fake_image))
    # same kernels on the same numbers; a fold of the older statistics or weights is 1e-3 or more away
    _check_l2(f_ex, ref, 1e-6, "f_ex against a freshly built encoder")


def test_train_loop_on_the_hard_mix_step(dev, host, capsys):
    """`train` with a ClusterMemory_Gradient and a 3-iteration loader in the [reid_batch, gan_dict] format (a TypeError before the
    step existed: the substitute loop handed `gan_inputs=` to a memory that does not take it)"""
    enc, gan, mem, opt, trainer = _gpu_parts(dev, host)
    trainer.train(0, _loader(host), opt, print_freq=1, train_iters=STEPS)
    out = capsys.readouterr().out
    assert out.count("Epoch: [0][") == STEPS and "train both gan and reid" not in out and "train adaptor and reid" not in out
    last, ref = _printed_losses(out)[-1], host["mix"]["losses"][-1]
    assert abs(last - ref) <= 1e-3 * abs(ref) + 5e-4, (last, ref)            # 5e-4: the print line's three decimals
    assert enc.training
    gan.use_adp = True
    trainer.sync_every_step = False
    capsys.readouterr()
    trainer.train(1, _loader(host), opt, print_freq=STEPS, train_iters=STEPS)
    out = capsys.readouterr().out
    assert out.startswith("train adaptor and reid") and out.count("Epoch: [1][") == 1


def test_train_reid_with_the_learnable_memory(dev, host, capsys):
    enc, gan, mem, opt, trainer = _gpu_parts(dev, host)
    capsys.readouterr()                                  # the constructors' own prints
    trainer.train_reid(0, _loader(host), opt, print_freq=1, train_iters=STEPS)
    out = capsys.readouterr().out
    assert out.startswith("warm up stage for reid") and out.count("Epoch: [0][") == STEPS
    for got, ref in zip(_printed_losses(out), host["warm"]):
        assert abs(got - ref) <= 1e-3 * abs(ref) + 5e-4, (got, ref)


def _shallow(dev, with_gan=True):
    """ResNet-18 + ClusterMemory + the joint trainer, seeded (tests.test_paths_gpu._cc_parts)"""
    from clustercontrast.trainers import ClusterContrastWithGANTrainer
    from dual_gan.models.models import create_model
    from tests.test_dualgan_gpu import _gan_opt
    enc, mem, opt, _, _, _ = _cc_parts(dev, 4)
    torch.manual_seed(1)
    gan = create_model(_gan_opt(model="AE"))
    trainer = ClusterContrastWithGANTrainer(enc, GAN=gan, memory=mem, opt=argparse.Namespace(num_instances=2, cl_temp=0.05))
    trainer.sync_every_step = True
    g = torch.Generator().manual_seed(6)
    items = []
    for i in range(3):
        gi = D.synth_dualgan_inputs(4, 64, 32, seed=20 + i)
        gi = {"Xs": gi["Xs"], "Ps": gi["Ps"], "Xs_path": ["a"] * 4, "gt_label": torch.zeros(4)}
        reid = (torch.randn(4, 3, 64, 32, generator=g), ["f"] * 4, torch.tensor([2, 2, 5, 5]), torch.zeros(4, dtype=torch.long),
                torch.arange(4))
        items.append([reid, gi])
    return enc, mem, opt, trainer, items


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_train_with_a_cluster_memory_keeps_todays_path(dev, capsys):
    """a ClusterMemory does not take `ex_f`: `train` is `train_all(joint=False)`, bit for bit"""
    enc1, mem1, opt1, tr1, items = _shallow(dev)
    enc2, mem2, opt2, tr2, _ = _shallow(dev)
    tr1.train(0, _Loader(items), opt1, print_freq=1, train_iters=3)
    out1 = capsys.readouterr().out
    tr2.train_all(0, _Loader(items), opt2, print_freq=1, train_iters=3, joint=False)
    out2 = capsys.readouterr().out
    assert "train both gan and reid" in out1 and _printed_losses(out1) == _printed_losses(out2) and len(_printed_losses(out1)) == 3
    assert _same_state(enc1, enc2) and torch.equal(mem1.features, mem2.features)


def test_train_reid_with_a_cluster_memory_is_the_cluster_contrast_step(dev, capsys):
    """the per-row loss of a ClusterMemory is averaged: the warm-up loop is ClusterContrastTrainer.step, bit for bit"""
    from clustercontrast.trainers import ClusterContrastTrainer
    enc1, mem1, opt1, tr1, items = _shallow(dev)
    enc2, mem2, opt2, _, _ = _shallow(dev)
    capsys.readouterr()                                  # the constructors' own prints
    tr1.train_reid(0, _Loader(items), opt1, print_freq=1, train_iters=3)
    out = capsys.readouterr().out
    assert out.startswith("warm up stage for reid")
    plain = ClusterContrastTrainer(enc2, mem2)
    ref = [plain.step(it[0][0].to(dev), it[0][2].to(dev), opt2).item() for it in items]
    # the print line shows the loss to three decimals
    assert _printed_losses(out) == [float("%.3f" % v) for v in ref]
    assert _same_state(enc1, enc2) and torch.equal(mem1.features, mem2.features)


def test_hard_mix_step_refuses_a_batch_of_broken_groups(dev, host):
    """a batch of 6 with groups of 4: ValueError before the encoder, the GAN or the optimizer is touched"""
    enc, gan, mem, opt, trainer = _gpu_parts(dev, host)
    x, labels, xs = host["items"][0]
    gan.set_input({"Xs": xs[:6]})
    state = copy.deepcopy(enc.state_dict())
    opt_state = copy.deepcopy(opt.state_dict())
    with pytest.raises(ValueError, match="groups of 4"):
        trainer.hard_mix_step(x[:6].to(dev), labels[:6].to(dev), opt, group_size=4)
    after = enc.state_dict()
    assert all(torch.equal(state[k], after[k]) for k in state)

    def same(a, b):
        if torch.is_tensor(a):
            return torch.equal(a, b)
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
        return a == b
    assert same(opt_state, opt.state_dict())
    assert all(p.grad is None for p in enc.parameters())
