"""not-gpu: the input staging of graph.StepGraph, as far as it can be checked without a device (the constructor opens a device
stream, so the object is built with __new__ and given the state its constructor sets; the static buffers are CPU tensors here).
  (1) non-tensor leaves of the inputs reach forward_loss as THIS call gave them, and are recorded in order;
  (2) a changed leaf, or a changed value of `key`, drops the graph and asks for one eager step before the next capture;
      unchanged leaves leave the graph alone;
  (3) nested dicts / lists / tuples keep their structure, the tensors in them are the static ones;
  (4) a changed tensor shape, dtype or nesting raises the error it always raised;
  (5) invalidate() drops the graph and keeps the static buffers."""
import pytest
import torch

from gpe_amd import graph


def _sg(key=None, warmup=2):
    sg = graph.StepGraph.__new__(graph.StepGraph)              # (the constructor opens a device stream)
    sg.device = torch.device('cpu')
    sg.key, sg.static_in, sg.leaves, sg.graph, sg.eager_left = key, None, None, None, warmup
    return sg


def _call(sg, seen):
    """what _forward does with the staged inputs"""
    sg.forward_loss = lambda *a: seen.append(a) or torch.zeros(())
    sg._forward()
    return seen[-1]


def test_non_tensor_leaves_are_those_of_the_current_call():
    sg, seen = _sg(), []
    x = torch.arange(4.0)
    sg._stage((x, 38, 'a'))
    a = _call(sg, seen)
    assert a[1:] == (38, 'a') and torch.equal(a[0], x) and a[0] is not x
    assert sg.leaves == [38, 'a']
    static = a[0]
    sg._stage((x + 1, 40, 'b'))
    a = _call(sg, seen)
    assert a[1:] == (40, 'b') and a[0] is static and torch.equal(static, x + 1)      # the same buffer, the new values
    assert sg.leaves == [40, 'b']


def test_a_changed_leaf_drops_the_graph_and_asks_for_an_eager_step():
    sg = _sg(warmup=0)
    x = torch.zeros(2)
    sg._stage((x, 39, None))
    assert sg.eager_left == 0                                  # the first call has nothing to differ from
    sg.graph = 'captured'
    sg._stage((x, 39, None))
    assert sg.graph == 'captured' and sg.eager_left == 0       # equal leaves: the graph stays
    sg._stage((x, 40, None))
    assert sg.graph is None and sg.eager_left == 1             # one eager step under the new value, then a capture
    sg.eager_left, sg.graph = 0, 'captured'
    sg._stage((x, 40.0, None))                                 # 40 == 40.0, but an int is not a float: compared with the type
    assert sg.graph is None and sg.eager_left == 1
    sg.eager_left, sg.graph = 0, 'captured'
    sg._stage((x, 40.0, False))
    assert sg.graph is None
    # during the warm-up a change costs no extra eager step
    sg.eager_left = 2
    sg._stage((x, 41.0, False))
    assert sg.eager_left == 2


def test_key_is_evaluated_at_every_step_and_compared_like_a_leaf():
    state = {'epoch': 38, 'calls': 0}

    def key():
        state['calls'] += 1
        return state['epoch'] >= 40

    sg = _sg(key=key, warmup=0)
    x = torch.zeros(2)
    sg._stage((x,))
    sg.graph = 'captured'
    state['epoch'] = 39
    sg._stage((x,))
    assert sg.graph == 'captured' and sg.leaves == [False] and state['calls'] == 2
    state['epoch'] = 40
    sg._stage((x,))
    assert sg.graph is None and sg.eager_left == 1 and sg.leaves == [True]
    sg.eager_left, sg.graph = 0, 'captured'
    state['epoch'] = 41
    sg._stage((x, ))
    assert sg.graph == 'captured' and state['calls'] == 4
    # the key stands behind the leaves of the inputs
    sg._stage((x,))
    assert sg.leaves == [True]


def test_leaves_that_cannot_be_compared_by_value_fall_back_to_identity():
    class Odd:
        def __eq__(self, other):
            raise TypeError('no truth value')

    sg = _sg(warmup=0)
    x, o = torch.zeros(2), Odd()
    sg._stage((x, o))
    sg.graph = 'captured'
    sg._stage((x, o))
    assert sg.graph == 'captured'
    sg._stage((x, Odd()))
    assert sg.graph is None


def test_nested_inputs_keep_their_structure():
    sg, seen = _sg(), []
    gt = {'outlines': torch.ones(2, 3), 'meta': [torch.zeros(1, dtype=torch.int64), ('tag', 7)], 'flag': True}
    feats = torch.full((2,), 5.0)
    sg._stage((feats, gt, 3))
    f, g, e = _call(sg, seen)
    assert e == 3 and isinstance(g, dict) and list(g) == ['outlines', 'meta', 'flag']
    assert isinstance(g['meta'], list) and isinstance(g['meta'][1], tuple) and g['meta'][1] == ('tag', 7) and g['flag'] is True
    assert torch.equal(g['outlines'], gt['outlines']) and g['outlines'] is not gt['outlines']
    assert g['meta'][0].dtype == torch.int64
    assert sg.leaves == ['tag', 7, True, 3]                    # in the order the tensors are walked
    statics = (f, g['outlines'], g['meta'][0])
    gt2 = {'outlines': torch.full((2, 3), 2.0), 'meta': [torch.ones(1, dtype=torch.int64), ('tag', 8)], 'flag': True}
    sg.graph = 'captured'
    sg._stage((feats * 2, gt2, 3))
    f, g, e = _call(sg, seen)
    assert all(a is b for a, b in zip((f, g['outlines'], g['meta'][0]), statics))
    assert torch.equal(f, feats * 2) and torch.equal(g['outlines'], gt2['outlines']) and int(g['meta'][0]) == 1
    assert g['meta'][1] == ('tag', 8) and sg.graph is None


def test_a_changed_shape_type_or_nesting_still_raises():
    sg = _sg()
    sg._stage((torch.zeros(2, 3), {'a': torch.zeros(4)}, 1))
    for bad in ((torch.zeros(3, 2), {'a': torch.zeros(4)}, 1),                     # shape
                (torch.zeros(2, 3, dtype=torch.float64), {'a': torch.zeros(4)}, 1),   # dtype
                (torch.zeros(2, 3), {'a': torch.zeros(4)}),                        # one argument fewer
                (torch.zeros(2, 3), {'b': torch.zeros(4)}, 1),                     # another key
                (torch.zeros(2, 3), [torch.zeros(4)], 1),                          # another container
                (torch.zeros(2, 3), {'a': torch.zeros(4)}, torch.zeros(1)),        # a tensor where a leaf was
                (torch.zeros(2, 3), {'a': torch.zeros(4), 'c': torch.zeros(1)}, 1)):
        with pytest.raises(RuntimeError, match='changed shape or type'):
            sg._stage(bad)
    sg._stage((torch.ones(2, 3), {'a': torch.ones(4)}, 1))                         # and the object is still usable
    assert sg.leaves == [1]


def test_invalidate_drops_the_graph_and_keeps_the_static_buffers():
    sg = _sg(warmup=0)
    sg._stage((torch.ones(3), 5))
    static = sg.static_in[0]
    sg.graph = 'captured'
    sg.invalidate()
    assert sg.graph is None and sg.static_in[0] is static and sg.eager_left == 0 and sg.leaves == [5]
    sg._stage((torch.zeros(3), 5))
    assert sg.static_in[0] is static and torch.equal(static, torch.zeros(3))
