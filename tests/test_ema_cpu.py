"""CPU tests of the weight average (rovit_hip/optim.py, ``ema_decay``): the decay schedule, the fp64 restatement of the recursion, argument
validation, the unchanged default, the two new entries of the C ABI and the deferred flat buffers of an optimizer built on a CPU model."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('rovit_adamw_ema_flat_multi', 'rovit_swap_flat_multi')


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


@pytest.fixture(scope='module')
def model():
    from models.rovit_kan import RoViTKAN
    torch.manual_seed(0)
    return RoViTKAN(pretrained=False)


def _reference_config(**extra):
    """The fields of the reference's TrainConfig / FlagsConfig that build_optimizer reads (configs/config.py:33-44): no ema_* field."""
    train = SimpleNamespace(batch_size=32, epochs=50, learning_rate=1e-4, weight_decay=1e-4, early_stop_patience=10, **extra)
    return SimpleNamespace(train=train, flags=SimpleNamespace(gradient_clip=1.0))


def test_decay_schedule_with_and_without_warmup(model):
    from rovit_hip.optim import RoViTAdamW
    warm = RoViTAdamW(model, ema_decay=0.999)
    assert warm.ema_warmup
    assert warm.ema_decay_at(1) == 2.0 / 11.0 and warm.ema_decay_at(2) == 3.0 / 12.0 and warm.ema_decay_at(90) == 91.0 / 100.0
    assert warm.ema_decay_at(8989) == 8990.0 / 8999.0 < 0.999          # (1 + t) / (10 + t) reaches 0.999 at t = 8 990
    assert warm.ema_decay_at(8991) == 0.999 and warm.ema_decay_at(10 ** 9) == 0.999
    ts = [warm.ema_decay_at(t) for t in range(1, 200)]
    assert ts == sorted(ts)
    flat = RoViTAdamW(model, ema_decay=0.999, ema_warmup=False)
    assert [flat.ema_decay_at(t) for t in (1, 2, 90, 10 ** 9)] == [0.999] * 4
    assert RoViTAdamW(model, ema_decay=0.0).ema_decay_at(5) == 0.0
    assert RoViTAdamW(model).ema_decay_at(5) == 0.0                       # off


@pytest.mark.parametrize('decay', [0.0, 0.5, 0.9, 0.999, 0.9999])
def test_reference_recursion_against_the_closed_form(decay):
    """Constant p: e_K = p + d^K (e_0 - p), with d = 1 - omd and omd the fp32 value the host computes from the fp32 decay."""
    from rovit_hip.optim import ema_reference
    rng = np.random.default_rng(3)
    p, e0 = rng.standard_normal(257), rng.standard_normal(257)
    omd = np.float64(np.float32(1.0 - np.float64(np.float32(decay))))
    d = 1.0 - omd
    e = e0.copy()
    for K in range(1, 25):
        e = ema_reference(e, p, decay)
        assert e.dtype == np.float64
        want = p + d ** K * (e0 - p)
        assert np.abs(e - want).max() <= 64 * np.finfo(np.float64).eps * max(np.abs(p).max(), np.abs(e0).max()), K
    assert np.array_equal(ema_reference(p, p, decay), p)                  # the lerp form leaves e == p where it is
    assert np.array_equal(ema_reference(e0.astype(np.float32), p.astype(np.float32), decay),
                          ema_reference(e0.astype(np.float32).astype(np.float64), p.astype(np.float32).astype(np.float64), decay))


def test_constructor_validation(model):
    from rovit_hip.optim import RoViTAdamW
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            RoViTAdamW(model, ema_decay=bad)
    for good in (0.0, 0.5, 0.9999):
        assert RoViTAdamW(model, ema_decay=good).ema_decay == good
    assert RoViTAdamW(model).ema_decay is None


def test_reference_config_builds_the_optimizer_it_builds_today(model):
    from rovit_hip import RovitHipError
    from rovit_hip.optim import RoViTAdamW, build_optimizer
    opt = build_optimizer(model, _reference_config())
    assert isinstance(opt, RoViTAdamW) and opt.ema_decay is None and opt.ema_flat is None and opt.o_ema is None
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups', 'rovit_flat'} and sd['rovit_flat'] is None
    flat = {'m_flat': torch.zeros(opt._bb_total), 'v_flat': torch.zeros(opt._bb_total), 'o_m': torch.zeros(opt._o_total),
            'o_v': torch.zeros(opt._o_total), 't': 3, 'segment_t': {s.name: 2 for s in opt.segments}}
    opt.load_state_dict(dict(sd, rovit_flat=flat))
    assert set(opt.state_dict()['rovit_flat']) == {'m_flat', 'v_flat', 'o_m', 'o_v', 't', 'segment_t'}
    for what in (opt.ema_state_dict, lambda: opt.load_ema_state_dict({}), lambda: opt.swap_ema().__enter__()):
        with pytest.raises(RovitHipError):
            what()
    on = build_optimizer(model, _reference_config(ema_decay=0.99, ema_warmup=False))
    assert on.ema_decay == 0.99 and on.ema_warmup is False
    assert build_optimizer(model, _reference_config(ema_decay=0.5)).ema_warmup is True


def test_new_entries_are_declared_bound_and_exported(native):
    import ctypes
    txt = open(os.path.join(ROOT, 'include', 'rovit_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW_ENTRIES:
        decl = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, txt)
        assert decl, f'{name} is not declared in include/rovit_hip.h'
        assert hasattr(lib, name), f'{name} declared but not exported'
        res, args = native.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(',')), name
    assert len(native.SIGNATURES['rovit_adamw_ema_flat_multi'][1]) == len(native.SIGNATURES['rovit_adamw_flat_multi'][1]) + 2
    assert native.load().rovit_version() == native.ABI_VERSION


def test_host_side_argument_checks_need_no_device(native):
    """Both NULL in a segment, a decay outside [0, 1) and a misaligned average are refused before anything is launched."""
    import ctypes as C
    lib = native.load()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += -base % 16
    one = lambda v: (C.c_void_p * 1)(v)
    n, lr, t = (C.c_size_t * 1)(8), (C.c_float * 1)(1e-3), (C.c_int * 1)(1)

    def run(g, ema, decay):
        return lib.rovit_adamw_ema_flat_multi(one(base), one(g), one(base), one(base), one(ema), n, lr, t, (C.c_float * 1)(decay), 1, None,
                                              0.9, 0.999, 1e-8, 1e-4, None)
    assert run(None, None, 0.5) == -3                                     # ROVIT_ERR_NULL
    assert run(base, base, 1.0) == -1 and run(base, base, -0.1) == -1 and run(None, base, float('nan')) == -1     # ROVIT_ERR_SHAPE
    assert run(base, base + 4, 0.5) == -2                                 # ROVIT_ERR_ALIGN
    assert lib.rovit_adamw_ema_flat_multi(one(base), one(base), one(base), one(base), one(base), n, lr, t, (C.c_float * 1)(0.5), 5, None,
                                          0.9, 0.999, 1e-8, 1e-4, None) == -1
    assert lib.rovit_swap_flat_multi(one(base), one(None), n, 1, None) == -3
    assert lib.rovit_swap_flat_multi(one(base), one(base + 4), n, 1, None) == -2
    assert lib.rovit_swap_flat_multi(one(base), one(base), n, 0, None) == -1


def test_an_ema_optimizer_on_a_cpu_model_defers_its_buffers(model):
    from rovit_hip import RovitHipError
    from rovit_hip.optim import RoViTAdamW
    opt = RoViTAdamW(model, ema_decay=0.99)
    assert opt.p_flat is None and opt.ema_flat is None and opt.o_ema is None
    assert opt.state_dict()['rovit_flat'] is None
    want = model.state_dict()
    got = opt.ema_state_dict()                                            # nothing stepped: the average is the parameters
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]) and got[k].data_ptr() != want[k].data_ptr(), k
    ema = torch.arange(opt._bb_total, dtype=torch.float32)
    o_ema = -torch.arange(opt._o_total, dtype=torch.float32)
    flat = {'m_flat': torch.zeros(opt._bb_total), 'v_flat': torch.zeros(opt._bb_total), 'o_m': torch.zeros(opt._o_total),
            'o_v': torch.zeros(opt._o_total), 't': 3, 'segment_t': {s.name: 2 for s in opt.segments}, 'ema_flat': ema, 'o_ema': o_ema}
    opt.load_state_dict(dict(opt.state_dict(), rovit_flat=flat))
    assert opt.p_flat is None and opt._pending_flat is flat               # applied when the buffers are built on the device
    assert opt.state_dict()['rovit_flat'] is flat
    got = opt.ema_state_dict()                                            # read out of the pending state, parameter by parameter
    p0 = opt.bb_params[0]
    name0 = next(k for k, p in model.named_parameters() if p is p0)
    assert torch.equal(got[name0].flatten(), ema[:p0.numel()])
    last = opt.segments[-1]
    name1 = next(k for k, p in model.named_parameters() if p is last.params[-1])
    assert torch.equal(got[name1].flatten(), o_ema[last.offsets[-1]:last.offsets[-1] + last.params[-1].numel()])
    for k, v in model.state_dict().items():
        if k not in dict(model.named_parameters()):
            assert torch.equal(got[k], v), k                              # buffers (the KAN knots) come from the model
    with pytest.raises(RovitHipError):
        with opt.swap_ema():
            pass
    assert not opt._swapped
