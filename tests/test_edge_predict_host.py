"""not-gpu: the host side of the encoder's prediction path (DynamicEdgeConv.predict / EdgeConvFeatures.predict / model.predict,
ops.edge_conv_predict, csrc/gpe_edge_predict.hip): argument checks that fire before any device check, the menu of the fused kernel
(ops.edge_predict_on_menu against the library's gpe_edge_predict_ok), and the declared / exported symbols."""
import copy
import ctypes
import os

import pytest
import torch

import gpe_amd
from gpe_amd import _lib, net_blocks, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _conv(C=3, H=200, F=112, k=16, hidden=1):
    return net_blocks.DynamicEdgeConv(net_blocks.MLP([2 * C] + [H] * (hidden + 1) + [F]), k=k)


def test_predict_in_training_mode_raises_before_any_device_check():
    x = torch.randn(2 * 32, 3)                                       # a CPU tensor: a device check would raise 'no CPU path'
    conv = _conv().train()
    with pytest.raises(RuntimeError, match=r'prediction path: call \.eval\(\) first'):
        conv.predict(x, 2, 32)
    ext = net_blocks.EdgeConvFeatures(40, {'k_neighbors': 4, 'EConv_hidden': 32, 'EConv_feature': 24}).train()
    with pytest.raises(RuntimeError, match=r'prediction path: call \.eval\(\) first'):
        ext.predict(x.view(2, 32, 3))
    fx = torch.load(os.path.join(GOLDEN, 'full3d_small.pt'), weights_only=False)
    model = gpe_amd.nets.GarmentFullPattern3D(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config'])).train()
    with pytest.raises(RuntimeError, match=r'prediction path: call \.eval\(\) first'):
        model.predict(fx['features'])


def test_unknown_route_raises_before_any_device_check():
    x = torch.randn(2 * 32, 3)
    conv = _conv().eval()
    with pytest.raises(ValueError, match='unknown route'):
        conv.predict(x, 2, 32, route='rows')
    with pytest.raises(ValueError, match='unknown route'):
        conv.train().predict(x, 2, 32, route='rows')                  # the route name is checked first, as in stitch_pairs
    ext = net_blocks.EdgeConvFeatures(40, {'k_neighbors': 4, 'EConv_hidden': 32, 'EConv_feature': 24}).eval()
    with pytest.raises(ValueError, match='unknown route'):
        ext.predict(x.view(2, 32, 3), route='nope')
    fx = torch.load(os.path.join(GOLDEN, 'segment3d_small.pt'), weights_only=False)
    model = gpe_amd.nets.GarmentSegmentPattern3D(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config'])).eval()
    with pytest.raises(ValueError, match='unknown route'):
        model.predict(fx['features'], route='rows')


def test_shape_and_menu_checks_come_before_the_device_check():
    conv = _conv(H=260).eval()
    with pytest.raises(ValueError, match="route='fused'"):
        conv.predict(torch.randn(64, 3), 2, 32, route='fused')
    conv = _conv(k=65).eval()
    with pytest.raises(ValueError, match="route='fused'"):
        conv.predict(torch.randn(160, 3), 2, 80, route='fused')
    conv = _conv().eval()
    with pytest.raises(ValueError, match='rows'):
        conv.predict(torch.randn(63, 3), 2, 32)
    with pytest.raises(ValueError, match='features'):
        conv.predict(torch.randn(64, 4), 2, 32)
    # everything in order: the next thing in the way is the device
    with pytest.raises(RuntimeError, match='no CPU path'):
        conv.predict(torch.randn(64, 3), 2, 32, route='fused')


# (H, F, k, hidden H x H layers) -> on the fused kernel's menu
MENU = [((200, 112, 5, 1), True), ((200, 112, 16, 1), True), ((200, 112, 20, 1), True), ((200, 112, 64, 1), True),
        ((200, 112, 65, 1), False), ((260, 112, 16, 1), False), ((30, 112, 16, 1), False), ((200, 112, 16, 4), False),
        ((200, 112, 16, 0), True), ((200, 112, 16, 3), True), ((256, 256, 1, 2), True), ((200, 150, 16, 1), True),
        ((200, 260, 16, 1), False), ((4, 4, 1, 0), True), ((200, 112, 0, 1), False)]


@pytest.mark.parametrize('case,expect', MENU)
def test_menu_truth_table(case, expect):
    H, F, k, hidden = case
    mlp = net_blocks.MLP([6] + [H] * (hidden + 1) + [F])
    assert ops.edge_predict_on_menu(mlp, k) is expect
    # the library's host-only query answers the same question (its trailing stream argument is ignored)
    assert _lib.lib().gpe_edge_predict_ok(k, H, F, hidden, None) == int(expect)


def test_menu_needs_equally_wide_hidden_layers():
    assert not ops.edge_predict_on_menu(net_blocks.MLP([6, 200, 100, 112]), 16)
    assert ops.edge_predict_on_menu(net_blocks.MLP([300, 200, 200, 112]), 16)     # the input width is the projection's business


def test_off_menu_arguments_are_rejected_without_a_launch():
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (k, H, F, n_hidden) off the menu -> -22 whatever the pointers; NULL operands on the menu -> -22 as well
    for k, H, F, nh in [(65, 200, 112, 1), (16, 260, 112, 1), (16, 30, 112, 1), (16, 200, 112, 4), (0, 200, 112, 1), (16, 200, 258, 1), (16, 200, 0, 1)]:
        assert l.gpe_edge_predict_fwd(p, 2 * H, p, 64, k, H, F, nh, p, None, None, p, 0, p, F, None) == -22
    assert l.gpe_edge_predict_fwd(None, 400, None, 64, 16, 200, 112, 1, None, None, None, None, 0, None, 112, None) == -22
    assert l.gpe_edge_predict_fwd(p, 400, p, 64, 16, 200, 112, 1, p, None, None, p, 3, p, 112, None) == -22        # aggr
    assert l.gpe_edge_predict_fwd(p, 396, p, 64, 16, 200, 112, 1, p, None, None, p, 0, p, 112, None) == -22        # ldpq < 2 H
    assert l.gpe_edge_predict_fwd(p, 400, p, 1 << 28, 16, 200, 112, 1, p, None, None, p, 0, p, 112, None) == -22   # BN k >= 2^31


def test_header_declares_and_library_exports_the_entry_points():
    sigs = _lib.parse_header()
    assert sigs['gpe_edge_predict_fwd'] == ('i', list('pipliiiippppipi') + ['p'])
    assert sigs['gpe_edge_predict_ok'] == ('i', list('iiii') + ['p'])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gpe_edge_predict_fwd', 'gpe_edge_predict_ok'):
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    assert _lib.lib().gpe_abi_version() == 7                              # an additive feature: no version bump
    src = open(_lib.HEADER_PATH).read()
    assert 'nn/net_blocks.py:43-47,124-135,174' in src[src.index('one DynamicEdgeConv layer at prediction time'):src.index('int gpe_edge_predict_ok')]
