"""GPU tests of the training epoch: rovit_joint_loss_mixed against rovit_joint_loss (bit for bit without a second label column), against
the reference's own two-call arithmetic and its fp64 restatement, the epoch record and its finalise, the absence of synchronisation in
``train_epoch``, and ``training.Trainer`` against the loop it replaces."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from training_fp64 import HEADS, LOSSES, WEIGHTS, check_against_fp64, make_batch, mixed_fp64

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
BATCHES = [1, 7, 300, 1000]          # 300 and 1000 make the kernel's 256-thread loop wrap


def dev():
    return torch.device('cuda:0')


# ---- 1. without a second label column it is the old kernel ------------------------------------------------------------------------------

def _old_and_new_kernel(out, ta, sev, alpha, stage, tb=None, lam=0.37):
    """Both entry points through the C ABI on the same inputs -> ((losses, grads) of rovit_joint_loss, of rovit_joint_loss_mixed).
    ``tb``: a second label column for rovit_joint_loss_mixed only; without one ``lam`` is not read."""
    from rovit_hip import native
    from rovit_hip.native import ptr
    gate = {'ordinal_logits': 2, 'mu': 3, 'log_var': 3, 'kan_severity': 4}
    h = [out[k].contiguous() if stage >= gate.get(k, 1) else None for k in HEADS]
    B, C = h[0].shape
    sev_i64 = sev.dtype == torch.int64
    res = []
    for new in (False, True):
        losses = torch.full((5,), float('nan'), device=dev())
        g = [None if t is None else torch.full_like(t, float('nan')) for t in h]
        if not new:
            native.call('rovit_joint_loss', *(ptr(t) for t in h), ptr(ta), ptr(sev), int(sev_i64), ptr(alpha), *(ptr(t) for t in g), ptr(losses),
                        B, C, *WEIGHTS, native.stream_ptr())
        else:
            d = native.TrainLoss()
            d.batch, d.num_classes, d.severity_is_int64, d.lam = B, C, int(sev_i64), lam
            d.lambda_ord, d.mu_unc, d.nu_kan, d.focal_gamma = WEIGHTS
            d.cls_logits, d.ordinal_logits, d.mu, d.log_var, d.kan_severity = (ptr(t) for t in h)
            d.class_targets_a, d.class_targets_b, d.severity_targets, d.focal_alpha = ptr(ta), ptr(tb), ptr(sev), ptr(alpha)
            d.d_cls, d.d_ord, d.d_mu, d.d_lv, d.d_kan = (ptr(t) for t in g)
            d.losses_out = ptr(losses)
            native.call('rovit_joint_loss_mixed', ctypes.byref(d), native.stream_ptr())
        res.append((losses, g))
    return res


@pytest.mark.parametrize('B', BATCHES)
def test_unmixed_is_bit_identical_to_the_old_kernel(B):
    out, ta, _, sev, alpha = make_batch(B, seed=B, device=dev())
    for stage in (1, 2, 3, 4):
        for a, s in ((None, sev.float()), (alpha, sev.float()), (None, sev), (alpha, sev)):          # focal_alpha; fp32 / int64 severity column
            (l_old, g_old), (l_new, g_new) = _old_and_new_kernel(out, ta, s, a, stage)
            assert torch.isfinite(l_old).all()
            assert torch.equal(l_old, l_new), (stage, l_old, l_new)
            for k, x, y in zip(HEADS, g_old, g_new):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (stage, k)


def test_unmixed_path_of_the_module_is_bit_identical_to_forward():
    from rovit_hip.losses import JointLoss
    out, ta, tb, sev, alpha = make_batch(300, seed=4, device=dev())
    lf = JointLoss(*WEIGHTS, focal_alpha=alpha)
    for stage in (1, 4):
        a = {k: v.clone().requires_grad_(True) for k, v in out.items()}
        want = lf(a, ta, sev, stage)
        (3.0 * want['total_loss']).backward()
        for lb, lam in ((None, 0.4), (tb, 1.0)):
            b = {k: v.clone().requires_grad_(True) for k, v in out.items()}
            got = lf.mixed(b, ta, lb, lam, sev, stage)
            (3.0 * got['total_loss']).backward()
            for k in LOSSES:
                assert torch.equal(got[k], want[k]), k
            for k in HEADS:
                assert (a[k].grad is None) == (b[k].grad is None) and (a[k].grad is None or torch.equal(a[k].grad, b[k].grad)), k


# ---- 2. mixed, against the reference's own arithmetic ---------------------------------------------------------------------------------

@pytest.mark.parametrize('B', BATCHES)
def test_mixed_matches_two_forward_calls_and_the_fp64_restatement(B):
    """trainer.py:104-111: lam * loss_fn(outputs, labels_a, ...)[k] + (1 - lam) * loss_fn(outputs, labels_b, ...)[k], upstream gradient 3.
    Tolerances of tests/test_gpu_loss.py: 1e-4 max(1, |v|) on losses, 1e-5 max(1, max |g|) on gradients.  The largest error of each
    comparison over all cases is printed."""
    from rovit_hip.losses import JointLoss
    out, ta, tb, sev, alpha = make_batch(B, seed=100 + B, device=dev())
    host = {k: v.cpu() for k, v in out.items()}
    worst = {'two calls': [0.0, 0.0], 'fp64': [0.0, 0.0]}
    for with_alpha in (False, True):
        lf = JointLoss(*WEIGHTS, focal_alpha=alpha if with_alpha else None)
        for stage in (1, 2, 3, 4):
            for lam in (0.0, 0.25, 0.9, 1.0):
                o = {k: v.clone().requires_grad_(True) for k, v in out.items()}
                got = lf.mixed(o, ta, tb, lam, sev, stage)
                (3.0 * got['total_loss']).backward()
                r = {k: v.clone().requires_grad_(True) for k, v in out.items()}
                la, lb = lf(r, ta, sev, stage), lf(r, tb, sev, stage)
                ref = {k: lam * la[k] + (1 - lam) * lb[k] for k in la}
                (3.0 * ref['total_loss']).backward()
                ref_l = {k: float(v.detach()) for k, v in ref.items()}
                ref_g = {k: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().double() for k, v in r.items()}
                grads = {k: o[k].grad for k in HEADS}
                e = check_against_fp64(got, grads, ref_l, ref_g, tag=('two calls', B, stage, lam))
                worst['two calls'] = [max(a, b) for a, b in zip(worst['two calls'], e)]
                f_l, f_g = mixed_fp64(host, ta.cpu(), tb.cpu(), lam, sev.cpu(), stage, WEIGHTS, alpha.cpu() if with_alpha else None)
                e = check_against_fp64(got, grads, f_l, f_g, upstream=3.0, tag=('fp64', B, stage, lam))
                worst['fp64'] = [max(a, b) for a, b in zip(worst['fp64'], e)]
    for k, (wl, wg) in worst.items():
        print(f'B={B} against {k}: worst loss error {wl * 1e-4:.2e} max(1,|v|), worst gradient error {wg * 1e-5:.2e} max(1,max|g|)')


def test_the_mixed_kernel_itself_at_lam_one():
    """``JointLoss.mixed`` takes the unmixed path at ``lam == 1.0``, so the two-column kernel meets that value only through the C ABI:
    1 * f(t_a) + 0 * f(t_b) is the old kernel's result within the loss tolerances, and an out-of-range label in column b still gives NaN
    (the reference's 0 * NaN)."""
    out, ta, tb, sev, alpha = make_batch(300, seed=12, device=dev())
    for stage in (1, 4):
        (l_old, g_old), (l_new, g_new) = _old_and_new_kernel(out, ta, sev.float(), alpha, stage, tb=tb, lam=1.0)
        ref_l = {k: float(v) for k, v in zip(LOSSES, l_old)}
        ref_g = {k: (torch.zeros_like(out[k]) if g is None else g).cpu().double() for k, g in zip(HEADS, g_old)}
        check_against_fp64(dict(zip(LOSSES, l_new)), dict(zip(HEADS, g_new)), ref_l, ref_g, tag=('lam 1', stage))
    bad_b = tb.clone()
    bad_b[5] = -1
    _, (l_bad, _) = _old_and_new_kernel(out, ta, sev.float(), alpha, 4, tb=bad_b, lam=1.0)
    assert torch.isnan(l_bad[0]) and torch.isnan(l_bad[4]) and torch.isfinite(l_bad[1:4]).all()


def test_an_out_of_range_label_in_column_b_poisons_the_class_loss_and_flags_the_row():
    from rovit_hip.losses import JointLoss
    from rovit_hip.training import TrainRecord
    from rovit_hip import native
    out, ta, tb, sev, _ = make_batch(300, seed=9, device=dev())
    lf, rec = JointLoss(*WEIGHTS), TrainRecord()
    good = lf.mixed(out, ta, tb, 0.25, sev, 4, record=rec)
    bad_b = tb.clone()
    bad_b[277] = 4
    bad = lf.mixed(out, ta, bad_b, 0.25, sev, 4, record=rec)
    assert torch.isfinite(good['cls_loss']) and torch.isnan(bad['cls_loss']) and torch.isnan(bad['total_loss'])
    assert torch.equal(bad['kan_loss'], good['kan_loss'])
    rows = rec.rows()
    assert rows[:, native.TRAIN_ROW_NONFINITE].tolist() == [0, 1] and rec.nonfinite_batches == 1


# ---- 3. record and finalise ----------------------------------------------------------------------------------------------------------

def _recorded_epoch(sizes):
    from rovit_hip.losses import JointLoss
    from rovit_hip.training import TrainRecord
    lf, rec = JointLoss(*WEIGHTS), TrainRecord(capacity=2)          # capacity 2: the table grows twice over five launches
    correct = total = 0
    per_batch = []
    for i, B in enumerate(sizes):
        out, ta, tb, sev, _ = make_batch(B, seed=50 + i, device=dev())
        per_batch.append(lf.mixed(out, ta, tb, 0.6, sev, 4, record=rec))
        correct += int(out['cls_logits'].argmax(1).eq(ta).sum())
        total += B
    return rec, per_batch, correct, total


def test_record_grows_counts_exactly_and_finalises_reproducibly():
    from rovit_hip import native
    from rovit_hip.training import result_block_from_rows
    sizes = (5, 300, 1, 64, 7)
    rec, per_batch, correct, total = _recorded_epoch(sizes)
    assert rec.n == total and rec.n_batches == 5 and rec._table.shape[0] >= 5
    blk = rec.result_block().copy()
    rows = rec.rows()
    assert rows[:, native.TRAIN_ROW_BATCH].tolist() == list(sizes)
    assert int(blk[native.TRAIN_N_ROWS]) == 5 and int(blk[native.TRAIN_SAMPLES]) == total and int(blk[native.TRAIN_CORRECT]) == correct
    assert int(blk[native.TRAIN_NONFINITE]) == 0
    x = rows[:, :5].copy().view(np.float32).astype(np.float64)
    for i, l in enumerate(per_batch):                       # the rows are the five values the launch returned
        assert x[i].tolist() == [float(l[k]) for k in LOSSES]
    sums = blk.view(np.float64)[native.TRAIN_LOSS:native.TRAIN_LOSS + 5]
    for k in range(5):                                      # fp64 rounding over at most 4 096 rows
        assert abs(sums[k] - x[:, k].sum()) <= 1e-12 * np.abs(x[:, k]).sum(), k
    assert np.array_equal(blk[:4], result_block_from_rows(rows)[:4])
    m = rec.compute()
    assert m['accuracy'] == 100. * correct / total and m['loss'] == sums[4] / 5
    again = _recorded_epoch(sizes)[0].result_block()
    assert np.array_equal(blk, again)


# ---- 4. no synchronisation before compute() -----------------------------------------------------------------------------------------------

def _setup(batch_size=8, synthetic=25, seed=0, lr=1e-4):
    from data.dataset import create_dataloaders
    from models.rovit_kan import RoViTKAN
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import build_optimizer
    torch.manual_seed(seed)
    np.random.seed(seed)
    loaders = create_dataloaders(None, None, CLASS_NAMES, SEVERITY, batch_size=batch_size, synthetic=synthetic, device=dev())
    model = RoViTKAN(pretrained=False).to(dev())
    cfg = SimpleNamespace(train=SimpleNamespace(learning_rate=lr, weight_decay=1e-4, epochs=4), flags=SimpleNamespace(gradient_clip=1.0))
    opt = build_optimizer(model, cfg)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0, focal_alpha=loaders[0].dataset.dataset.get_class_weights().to(dev()), num_classes=4)
    return model, loaders, opt, loss_fn


MIX = dict(use_cutmix=True, use_mixup=True, cutmix_alpha=1.0, mixup_alpha=0.2)
NO_MIX = dict(use_cutmix=False, use_mixup=False, cutmix_alpha=1.0, mixup_alpha=0.2)


def test_train_epoch_never_synchronises_and_compute_copies_once(monkeypatch):
    from rovit_hip import training
    from rovit_hip.training import TrainRecord, train_epoch
    model, (train_loader, _, _), opt, loss_fn = _setup(batch_size=8, synthetic=25)          # 20 training images: batches of 8, 8, 4
    assert len(train_loader) == 3 and not next(iter(train_loader))[1].is_cuda              # host labels, like a DataLoader's
    train_epoch(model, train_loader, opt, loss_fn, 4, **MIX)                               # warm: allocator pools, code objects
    rec = TrainRecord()
    monkeypatch.setattr(TrainRecord, 'compute', lambda self: {})                           # the epoch body alone
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        train_epoch(model, train_loader, opt, loss_fn, 4, record=rec, **MIX)
        monkeypatch.undo()
        with pytest.raises(RuntimeError):                                                  # compute() is where the epoch synchronises
            rec.compute()
    finally:
        torch.cuda.set_sync_debug_mode('default')
        monkeypatch.undo()
    assert rec.n == 20 and rec.n_batches == 3
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    m = rec.compute()
    monkeypatch.undo()
    assert copies == [(training.native.TRAIN_RESULT_WORDS,)], copies                        # one device-to-host copy: the result block
    assert np.isfinite(m['loss']) and 0.0 <= m['accuracy'] <= 100.0


# ---- 5. Trainer against the loop it replaces -----------------------------------------------------------------------------------------------

def _reference_epoch(model, loader, optimizer, loss_fn, stage, use_mix, max_batches=None, keep=None):
    """The body of the reference's Trainer.train_epoch (training/trainer.py:54-181) on the drop-in pieces, as
    tests/test_gpu_round2.py::_trainer_shaped_epoch restates it, returning the trainer's six metrics."""
    from data.transforms import cutmix_or_mixup
    device = dev()
    model.train()
    model.curriculum_stage = stage
    sums = dict.fromkeys(LOSSES, 0.0)
    correct = total = nb = 0
    for images, class_labels, severity_labels in loader:
        images, class_labels, severity_labels = images.to(device), class_labels.to(device), severity_labels.to(device)
        if use_mix:
            images, la, lb, lam = cutmix_or_mixup(images, class_labels, **MIX)
        outputs = model(images)
        if use_mix:
            a, b = loss_fn(outputs, la, severity_labels, stage), loss_fn(outputs, lb, severity_labels, stage)
            losses = {k: lam * a[k] + (1 - lam) * b[k] for k in a}
        else:
            losses = loss_fn(outputs, class_labels, severity_labels, stage)
        loss = losses['total_loss']
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()                                     # RoViTAdamW: the clip is inside
        for k in LOSSES:
            sums[k] += losses[k].item()
        _, predicted = outputs['cls_logits'].max(1)
        total += class_labels.size(0)
        correct += predicted.eq(class_labels).sum().item()
        nb += 1
        if keep is not None:
            keep.append((outputs['cls_logits'].detach().clone(), {k: float(v.detach()) for k, v in losses.items()}))
        if max_batches is not None and nb >= max_batches:
            break
    m = {('loss' if k == 'total_loss' else k): v / nb for k, v in sums.items()}
    m['accuracy'] = 100. * correct / total
    return m


def _run_four_stages(new):
    from rovit_hip.training import train_epoch
    model, (train_loader, _, _), opt, loss_fn = _setup(batch_size=8, synthetic=30, lr=1e-3)          # 24 training images: three steps per stage
    assert len(train_loader) == 3
    metrics = []
    for stage in (1, 2, 3, 4):
        if new:
            metrics.append(train_epoch(model, train_loader, opt, loss_fn, stage, mix_loss=True, gradient_clip=1.0, **NO_MIX))
        else:
            metrics.append(_reference_epoch(model, train_loader, opt, loss_fn, stage, use_mix=False))
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in model.named_parameters()}, metrics


def test_train_epoch_without_mixing_reproduces_the_replaced_loop_bit_for_bit():
    p1, m1 = _run_four_stages(new=False)
    p2, m2 = _run_four_stages(new=False)
    assert all(torch.equal(p1[n], p2[n]) for n in p1) and m1 == m2, 'the replaced loop does not reproduce itself'
    p3, m3 = _run_four_stages(new=True)
    assert all(torch.isfinite(p).all() for p in p3.values())
    for n in p1:
        assert torch.equal(p1[n], p3[n]), n
    for want, got in zip(m1, m3):
        assert set(got) == set(want) == {'loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'accuracy'}
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])


def test_first_mixed_step_matches_the_replaced_loop():
    from rovit_hip.training import train_epoch
    model, (train_loader, _, _), opt, loss_fn = _setup(batch_size=8, synthetic=30)
    kept = []
    _reference_epoch(model, train_loader, opt, loss_fn, 4, use_mix=True, max_batches=1, keep=kept)
    want_logits, want = kept[0]
    model, (train_loader, _, _), opt, loss_fn = _setup(batch_size=8, synthetic=30)
    seen = []
    real = loss_fn.mixed

    def spy(outputs, la, lb, lam, *a, **k):
        losses = real(outputs, la, lb, lam, *a, **k)
        seen.append((outputs['cls_logits'].detach().clone(), lb is not None, {n: float(v.detach()) for n, v in losses.items()}))
        return losses
    loss_fn.mixed = spy
    first = [next(iter(train_loader))]
    m = train_epoch(model, first, opt, loss_fn, 4, mix_loss=True, gradient_clip=1.0, **MIX)
    got_logits, had_b, got = seen[0]
    assert had_b
    assert torch.equal(got_logits, want_logits)              # the forward is untouched: same seeds, same mix, same logits
    for k in LOSSES:
        assert abs(got[k] - want[k]) < 1e-4 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert abs(m['loss'] - got['total_loss']) <= 1e-6 * abs(got['total_loss'])


def _stage_for_epoch(epoch):          # module level: the config is pickled into the checkpoint
    return min(4, epoch + 2)


def test_trainer_fit_end_to_end_and_checkpoint_round_trip(tmp_path):
    from models.rovit_kan import RoViTKAN
    from training import JointLoss, Trainer, build_optimizer, build_scheduler

    def make(seed):
        from data.dataset import create_dataloaders
        torch.manual_seed(seed)
        np.random.seed(seed)
        tr, va, _ = create_dataloaders(None, None, CLASS_NAMES, SEVERITY, batch_size=8, synthetic=30, device=dev())
        cfg = SimpleNamespace(
            train=SimpleNamespace(learning_rate=1e-4, weight_decay=1e-4, epochs=2, early_stop_patience=5),
            flags=SimpleNamespace(use_cutmix=True, use_mixup=True, cutmix_alpha=1.0, mixup_alpha=0.2, mixed_precision=True, gradient_clip=1.0,
                                  freeze_backbone_epochs=1, curriculum=True),
            paths=SimpleNamespace(checkpoints_dir=tmp_path), get_stage_for_epoch=_stage_for_epoch)
        model = RoViTKAN(pretrained=False)
        opt = build_optimizer(model, cfg)                    # before the model moves to the device, as scripts/train.py does
        return Trainer(model, tr, va, opt, build_scheduler(opt, cfg), JointLoss(), cfg, dev())
    t = make(0)
    history = t.fit()
    assert all(len(v) == 2 and np.isfinite(v).all() for v in history.values())
    assert t.last_train_record.n == 24 and t.last_train_record.n_batches == 3 and t.last_train_record.nonfinite_batches == 0
    assert t.model.curriculum_stage == 4 and t.best_epoch in (1, 2)
    path = tmp_path / 'best_model.pth'
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ck) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_val_loss', 'metrics', 'config'}
    fresh = make(7)
    fresh.load_checkpoint(path)
    assert fresh.best_val_loss == t.best_val_loss
    want = RoViTKAN(pretrained=False)
    want.load_state_dict(ck['model_state_dict'])
    want = want.to(dev()).eval()
    fresh.model.eval()
    x = torch.randn(4, 3, 224, 224, device=dev())
    with torch.no_grad():
        a, b = fresh.model(x), want(x)
        if t.best_epoch == 2:                                # the saved model is the trained one
            t.model.eval()
            c = t.model(x)
    for k in HEADS:
        assert torch.equal(a[k], b[k]), k
        if t.best_epoch == 2:
            assert torch.equal(a[k], c[k]), k
