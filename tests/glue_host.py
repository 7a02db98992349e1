"""What the not-gpu glue tests share (test_mlp_glue_host.py, test_rnn_glue_host.py): stand-ins for arguments, the parameter names a
declaration of include/gpe_hip.h gives, a recorder in L.call's place, and the position-by-position check of a recorded call."""
import re

import pytest

from gpe_amd import _lib, ops


class Named:
    """a stand-in for one argument: equal to nothing but itself"""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return '<%s>' % self.name


class Ptrs:
    """what a recorder in ops._ptr_array's place returns: the list it was given, tagged"""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def __repr__(self):
        return 'Ptrs(%r)' % (self.tensors,)


def named(*names):
    return {n: Named(n) for n in names}


def declared(entry):
    """the parameter names of `entry` as include/gpe_hip.h declares them"""
    src = re.sub(r'/\*.*?\*/', ' ', open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % entry, src)
    names = [re.search(r'(\w+)\s*$', p).group(1) for p in m.group(1).split(',')]
    assert len(names) == len(_lib.parse_header()[entry][1]) and names[-1] == 'stream'
    return names


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    monkeypatch.setattr(ops.L, 'call', lambda name, *args: calls.append((name, args)))
    return calls


def check(recorded, entry, expect):
    """the one call recorded is `entry`, and every position carries what `expect` has under the declaration's name for it: a stand-in or
    None itself, a Ptrs of the same tensors in the same order, an int of that value"""
    names = declared(entry)[:-1]                               # (L.call appends the stream)
    assert len(recorded) == 1 and recorded[0][0] == entry
    args = recorded[0][1]
    assert len(args) == len(names)
    assert set(expect) == set(names)
    for pos, (name, arg) in enumerate(zip(names, args)):
        want = expect[name]
        if isinstance(want, Ptrs):
            assert isinstance(arg, Ptrs) and len(arg.tensors) == len(want.tensors), (pos, name, arg)
            assert all(a is b for a, b in zip(arg.tensors, want.tensors)), (pos, name, arg)
        else:
            assert (arg is want) if isinstance(want, Named) or want is None else (type(arg) is int and arg == want), (pos, name, arg)
    del recorded[:]


def missing_each(wrapper, kw, recorded, optional=()):
    for name in kw:
        if name not in optional:
            with pytest.raises(TypeError):
                wrapper(**{k: v for k, v in kw.items() if k != name})
    with pytest.raises(TypeError):
        wrapper(*kw.values())                                  # (keywords only: a position cannot be mistaken for another)
    assert recorded == []
