"""The layout of the ops modules (DESIGN.md "ops modules"): ops.py is the facade and the ONE home of every name that callers
rebind; _opbase and the leaves ops_stitch / ops_losses / ops_data / ops_eval hold code that reads none of them and are re-exported
by ops.  No GPU: imports, code objects and syntax trees only.

What "reads a switch" means here: a code object that reaches the name as a GLOBAL (LOAD_GLOBAL / LOAD_NAME / STORE_* / DELETE_* in
its bytecode).  `co_names` alone would not do: it also lists attribute names, and `ops.CAPTURE = self` in graph.py, an assignment
THROUGH the facade, is exactly the access that has to keep working."""
import ast
import dis
import importlib
import os
import subprocess
import sys
import types

import pytest

import gpe_amd
from gpe_amd import _opbase, ops, ops_data, ops_eval, ops_losses, ops_stitch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.abspath(ops.__file__))
LEAVES = (ops_stitch, ops_losses, ops_data, ops_eval)
# name -> who rebinds it (DESIGN.md keeps the same table)
SWITCHES = ('SIDE_GRADS', 'SIDE_MIN_EDGES', '_LAST_EDGES', 'CAPTURE', 'HOST_DRAWN', 'RNN_WS_HOOK', 'WEIGHTS_EPOCH', '_HALF_ACT_GUARD',
            'planned_planes', '_ptr_array')
GLOBAL_OPS = {'LOAD_GLOBAL', 'LOAD_NAME', 'STORE_GLOBAL', 'STORE_NAME', 'DELETE_GLOBAL', 'DELETE_NAME'}


def _package_modules():
    return [importlib.import_module('gpe_amd.' + f[:-3]) for f in sorted(os.listdir(PKG)) if f.endswith('.py') and f != '__init__.py']


def _codes(code):
    yield code
    for c in code.co_consts:
        if isinstance(c, types.CodeType):
            yield from _codes(c)


def _switch_reads(code):
    """the switches a code object, or one nested in it, reaches as globals"""
    return sorted({i.argval for c in _codes(code) if set(c.co_names) & set(SWITCHES)
                   for i in dis.get_instructions(c) if i.opname in GLOBAL_OPS and i.argval in SWITCHES})


def _functions(module):
    """every function and method defined in `module` (properties, static and class methods unwrapped; nested code rides along)"""
    for v in vars(module).values():
        if isinstance(v, types.FunctionType) and v.__module__ == module.__name__:
            yield v
        elif isinstance(v, type) and v.__module__ == module.__name__:
            for m in vars(v).values():
                m = getattr(m, '__func__', m)
                for f in ((m.fget, m.fset, m.fdel) if isinstance(m, property) else (m,)):
                    if isinstance(f, types.FunctionType):
                        yield f


def _top_names(module):
    """the names a module's own top-level statements define (def, class, assignment), in order, repeats included"""
    out = []
    for s in ast.parse(open(module.__file__).read()).body:
        if isinstance(s, (ast.FunctionDef, ast.ClassDef)):
            out.append(s.name)
        elif isinstance(s, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
            out += [t.id for t in ast.walk(s) if isinstance(t, ast.Name) and isinstance(t.ctx, ast.Store)]
    return out


def _misplaced(modules):
    """(module, function, switches) of every function that reads a switch and whose globals are not those of ops"""
    return [(m.__name__, f.__qualname__, _switch_reads(f.__code__)) for m in modules for f in _functions(m)
            if _switch_reads(f.__code__) and f.__globals__ is not vars(ops)]


def test_every_recorded_name_resolves_on_ops():
    """tests/golden/ops_names.txt: every public attribute of ops that is not a module, recorded before the split, then the
    underscore names that tests, scripts and other modules of the package use"""
    names = open(os.path.join(REPO, 'tests', 'golden', 'ops_names.txt')).read().split()
    assert len(names) > 200 and len(set(names)) == len(names)
    assert [n for n in names if not hasattr(ops, n)] == []


def test_reexports_are_the_same_objects():
    for leaf in LEAVES:
        assert leaf.__all__ and len(set(leaf.__all__)) == len(leaf.__all__)
        assert sorted(leaf.__all__) == sorted(n for n in _top_names(leaf) if not n.startswith('_')), leaf.__name__   # the star is exact
        for n in leaf.__all__:
            assert getattr(ops, n) is getattr(leaf, n), (leaf.__name__, n)
    base = [n for n, v in vars(_opbase).items() if not n.startswith('__') and not isinstance(v, types.ModuleType) and n != 'torch']
    imported = [n for n in base if n in vars(ops)]
    assert {'F32', 'F64', '_WS', '_rows2d', '_rows3d', '_workspace', '_ticket', 'round_up', 'edge_workspace', 'f16x3_words'} <= set(imported)
    for n in imported:
        assert getattr(ops, n) is getattr(_opbase, n), n
    for m in (_opbase, ops) + LEAVES:                   # one L: what tests/glue_host.py patches as ops.L.call is what every module calls
        assert m.L is gpe_amd._lib


def test_switches_have_one_home():
    modules = _package_modules()
    assert {m.__name__ for m in modules} >= {'gpe_amd.ops', 'gpe_amd._opbase', 'gpe_amd.graph'} | {l.__name__ for l in LEAVES}
    for n in SWITCHES:
        assert n in vars(ops), n
        assert [m.__name__ for m in modules if m is not ops and n in vars(m)] == [], n
    # the walker sees the readers it is there for: these live in ops and do read a switch
    readers = {f.__qualname__: _switch_reads(f.__code__) for f in _functions(ops)}
    assert readers['_side_ok'] == ['SIDE_GRADS', 'SIDE_MIN_EDGES'] and readers['bump_weights_epoch'] == ['WEIGHTS_EPOCH']
    assert '_LAST_EDGES' in readers['side_grads'] and '_HALF_ACT_GUARD' in readers['set_half_act_guard']
    assert _misplaced(modules) == []
    for m in modules:
        tree = ast.parse(open(m.__file__).read())
        globs = [n for n in ast.walk(tree) if isinstance(n, ast.Global)]
        if m is not ops:                                # (_lib.py keeps `global _lib`, the handle of the loaded library: its own state)
            assert [n.lineno for n in globs if m is not gpe_amd._lib or set(n.names) != {'_lib'}] == [], m.__name__
        if m is _opbase or m in LEAVES:                 # no name there is assigned twice: caches are mutated, never rebound
            assert len(_top_names(m)) == len(set(_top_names(m))), m.__name__


def test_the_walker_rejects_a_reader_outside_ops():
    """the wrong variant: a module that reads SIDE_GRADS itself (directly, in a nested function and in a method) is named; one
    that goes through the facade is not"""
    wrong = types.ModuleType('gpe_amd.ops_wrong')
    exec(compile('SIDE_GRADS = True\n'
                 'def direct(edges):\n    return bool(SIDE_GRADS and edges)\n'
                 'def nested():\n    return [(lambda: CAPTURE)() for _ in range(1)]\n'
                 'class C:\n    @staticmethod\n    def forward(ctx):\n        global WEIGHTS_EPOCH\n        WEIGHTS_EPOCH = 1\n'
                 'def through_the_facade(ops):\n    ops.SIDE_GRADS = False\n    return ops.HOST_DRAWN\n', 'ops_wrong.py', 'exec'),
         vars(wrong))
    for f in (wrong.direct, wrong.nested, wrong.C.forward, wrong.through_the_facade):
        f.__module__ = wrong.__name__
    wrong.C.__module__ = wrong.__name__
    assert _misplaced([wrong]) == [('gpe_amd.ops_wrong', 'direct', ['SIDE_GRADS']), ('gpe_amd.ops_wrong', 'nested', ['CAPTURE']),
                                   ('gpe_amd.ops_wrong', 'C.forward', ['WEIGHTS_EPOCH'])]


@pytest.mark.parametrize('first', ['import gpe_amd',
                                   'import gpe_amd; from gpe_amd import ops_eval, ops_stitch',
                                   "import importlib; importlib.import_module('gpe_amd.ops_stitch')"])
def test_fresh_process_import_order(first):
    """the cycle ops -> ops_stitch -> ops closes in every order a caller can start it, because the package imports ops first"""
    code = (first + "; import sys; ops, leaf = sys.modules['gpe_amd.ops'], sys.modules['gpe_amd.ops_stitch']\n"
            "assert ops.stitch_pairs is leaf.stitch_pairs and leaf.dense_mlp is ops.dense_mlp and ops.FrameworkAccumulator\n"
            "import torch; assert not torch.cuda.is_initialized()\nprint('same', ops.stitch_pairs is leaf.stitch_pairs)")
    r = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'same True', r.stdout + r.stderr


def test_module_sizes():
    """ops.py under 2000 lines, no new module over 700; together they exceed the 3300 lines of the file they were cut from only
    by their heads (docstring, imports, __all__) and the re-export"""
    lines = {m.__name__: len(open(m.__file__).read().split('\n')) - 1 for m in (_opbase, ops) + LEAVES}
    assert lines['gpe_amd.ops'] < 2000
    assert all(n <= 700 for name, n in lines.items() if name != 'gpe_amd.ops'), lines
    assert sum(lines.values()) <= 3300 + 120, lines
