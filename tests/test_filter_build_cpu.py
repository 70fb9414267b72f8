"""Filter layouts built by the layout kernels (filter build mode 'device') against the host functions, on the emulator: tests/filter_build_cases.py"""
import pytest

import filter_build_cases as fb
from realtime_yukarin_amd.netspec import NetDesc


@pytest.mark.parametrize('name,shape,kw', fb.LAYERS_1D, ids=[c[0] for c in fb.LAYERS_1D])
def test_layer_layouts_1d_emu(emu_ctx, name, shape, kw):
    assert fb.check_layer(emu_ctx, name, shape, kw, seed=11) == ['w1d', 'w1os']


@pytest.mark.parametrize('name,shape,kw', fb.LAYERS_2D, ids=[c[0] for c in fb.LAYERS_2D])
def test_layer_layouts_2d_emu(emu_ctx, name, shape, kw):
    fb.check_layer(emu_ctx, name, shape, kw, seed=21, expect=fb.EXPECT_2D[name])


def test_predictor_layouts_stage1_poisoned_emu(emu_ctx, monkeypatch):
    """every float of every layout of a stage-1 predictor (k3, k4 s2, k1, deconvolutions over two sources), the counters, the arena bytes: RY_POISON=1"""
    assert fb.check_predictor_layouts(emu_ctx, NetDesc(1, 3, 5, 16, 3), 1, 31, monkeypatch) == ['w1d', 'w1os']


def test_predictor_layouts_stage2_poisoned_emu(emu_ctx, monkeypatch):
    """... of a stage-2 predictor with every stage-2 kind, the output-stationary one by a lowered RY_OS2_MINW"""
    assert fb.check_predictor_layouts(emu_ctx, fb.S2_SMALL, fb.S2_WIDTH, 41, monkeypatch, os2_minw=1) == ['w2os', 'wdir', 'wig', 'wwin']


def test_forward_bits_clones_and_mode_switch_emu(emu_ctx, monkeypatch):
    assert fb.check_forward_bits(emu_ctx, monkeypatch)


def test_refusals_emu(emu_ctx, monkeypatch):
    fb.check_refusals(emu_ctx, monkeypatch)
