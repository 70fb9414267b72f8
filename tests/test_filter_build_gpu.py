"""Filter layouts built on the card (filter build mode 'device') against the host functions: tests/filter_build_cases.py on the MI355X"""
import pytest

import filter_build_cases as fb
from realtime_yukarin_amd.netspec import NetDesc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name,shape,kw', fb.LAYERS_1D, ids=[c[0] for c in fb.LAYERS_1D])
def test_layer_layouts_1d_gpu(gpu_ctx, name, shape, kw):
    assert fb.check_layer(gpu_ctx, name, shape, kw, seed=11) == ['w1d', 'w1os']


@pytest.mark.parametrize('name,shape,kw', fb.LAYERS_2D, ids=[c[0] for c in fb.LAYERS_2D])
def test_layer_layouts_2d_gpu(gpu_ctx, name, shape, kw):
    fb.check_layer(gpu_ctx, name, shape, kw, seed=21, expect=fb.EXPECT_2D[name])


def test_syn64_largest_layer_gpu(gpu_ctx, monkeypatch):
    """the full-size layer: 8.4 M filter floats, 18.9 M Winograd floats, every kind it has, on poisoned memory"""
    name, shape, kw = fb.syn64_largest_layer()
    try:
        fb.poison(gpu_ctx, monkeypatch)
        assert fb.check_layer(gpu_ctx, name, shape, kw, seed=51) == ['w2os', 'wdir', 'wig', 'wwin']
    finally:
        fb.poison(gpu_ctx, monkeypatch, False)


def test_predictor_layouts_stage1_poisoned_gpu(gpu_ctx, monkeypatch):
    assert fb.check_predictor_layouts(gpu_ctx, NetDesc(1, 3, 5, 16, 3), 1, 31, monkeypatch) == ['w1d', 'w1os']


def test_predictor_layouts_stage2_poisoned_gpu(gpu_ctx, monkeypatch):
    assert fb.check_predictor_layouts(gpu_ctx, fb.S2_SMALL, fb.S2_WIDTH, 41, monkeypatch, os2_minw=1) == ['w2os', 'wdir', 'wig', 'wwin']


def test_forward_bits_clones_and_mode_switch_gpu(gpu_ctx, monkeypatch):
    assert fb.check_forward_bits(gpu_ctx, monkeypatch)


def test_refusals_gpu(gpu_ctx, monkeypatch):
    fb.check_refusals(gpu_ctx, monkeypatch)
