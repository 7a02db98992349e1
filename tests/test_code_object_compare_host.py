"""not-gpu: scripts/compare_code_objects.py, the tool that holds a move of kernel sources to "no kernel's machine code changed"
(profiles/csrc_split.md).  A two-kernel source is compiled for gfx950 three ways — as one file, as two files with one kernel each,
and with a constant changed in one kernel — and the tool must call the first two the same build (kernels are matched by name across
a build, and a descriptor's entry offset, which depends on where the kernel sits in its code object, is masked), name exactly the
changed kernel in the third, and report a kernel that only one side has.  No GPU: nothing is loaded or run."""
import concurrent.futures
import importlib.util
import os
import subprocess
import sys

import pytest

from gpe_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'scripts', 'compare_code_objects.py')

HEAD = '#include <hip/hip_runtime.h>\n'
AXPY = '''extern "C" __global__ void cmp_axpy(const float* __restrict__ x, float* __restrict__ y, float a, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a * x[i] + y[i];
}
'''
# (longer than cmp_axpy and behind it in the one-file build: its distance from its descriptor differs between the builds)
SCALE = '''extern "C" __global__ void cmp_scale(const float* __restrict__ x, float* __restrict__ y, long n)
{
    __shared__ float red[64];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    red[threadIdx.x & 63] = (i < n) ? x[i] : 0.f;
    __syncthreads();
    if (i < n) y[i] = %s * x[i] + red[(threadIdx.x + 1) & 63];
}
'''
BUILDS = {'one': {'both.hip': HEAD + AXPY + SCALE % '3.f'},
          'two': {'first.hip': HEAD + AXPY, 'second.hip': HEAD + SCALE % '3.f'},
          'changed': {'both.hip': HEAD + AXPY + SCALE % '5.f'},
          'axpy_only': {'first.hip': HEAD + AXPY}}


def _tool():
    spec = importlib.util.spec_from_file_location('compare_code_objects', TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _compile(job):
    src, obj = job
    r = subprocess.run([build.HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', src, '-o', obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    """directory of each build's objects; the sources are compiled once, side by side"""
    assert os.path.exists(build.HIPCC), 'no hipcc at %s' % build.HIPCC
    top = tmp_path_factory.mktemp('code_objects')
    jobs, dirs = [], {}
    for name, files in BUILDS.items():
        d = top / name
        d.mkdir()
        dirs[name] = str(d)
        for fname, text in files.items():
            (d / fname).write_text(text)
            jobs.append((str(d / fname), str(d / (fname[:-4] + '.o'))))
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(_compile, jobs))
    return dirs


def test_one_file_and_two_files_are_the_same_build(builds, tmp_path):
    tool = _tool()
    only_a, only_b, code, desc, counts = tool.compare(builds['one'], builds['two'])
    assert (only_a, only_b, code, desc) == ([], [], [], [])
    assert counts == (1, 2, 2, 2)                       # objects and kernels per side: both kernels were found on both
    # the masked field is what differs: without the mask the second kernel's descriptor would not match
    one = dict((n, kd) for n, _, kd in tool.object_kernels(os.path.join(builds['one'], 'both.o'), str(tmp_path)))
    assert sorted(one) == ['cmp_axpy', 'cmp_scale'] and all(len(kd) == 64 and kd[16:24] == bytes(8) for kd in one.values())


def test_a_changed_constant_names_its_kernel_and_no_other(builds):
    only_a, only_b, code, desc, _ = _tool().compare(builds['one'], builds['changed'])
    assert (only_a, only_b, desc) == ([], [], [])
    assert [c[0] for c in code] == ['cmp_scale']
    # ... and against the two-file build as well: the match is by name, not by file
    only_a, only_b, code, desc, _ = _tool().compare(builds['two'], builds['changed'])
    assert (only_a, only_b, desc) == ([], [], []) and [c[0] for c in code] == ['cmp_scale']


def test_a_kernel_on_one_side_only_is_reported(builds):
    tool = _tool()
    only_a, only_b, code, desc, _ = tool.compare(builds['one'], builds['axpy_only'])
    assert (only_a, only_b, code, desc) == (['cmp_scale'], [], [], [])
    only_a, only_b, code, desc, _ = tool.compare(builds['axpy_only'], builds['two'])
    assert (only_a, only_b, code, desc) == ([], ['cmp_scale'], [], [])


@pytest.mark.parametrize('other, status', [('two', 0), ('changed', 1), ('axpy_only', 1)])
def test_exit_status_is_zero_only_for_the_same_build(builds, other, status):
    r = subprocess.run([sys.executable, TOOL, builds['one'], builds[other]], capture_output=True, text=True)
    assert r.returncode == status, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith('SAME' if status == 0 else 'DIFFERENT')
