"""garment-pattern-estimation_amd — MI355X-native (gfx950) implementation of the NeuralTailor hot path:
point-cloud encoder (dynamic-kNN EdgeConv) -> panel-sequence decoder (LSTM), forward + backward.

`nets` / `net_blocks` mirror the class names, constructor signatures, config keys, output dict and state-dict
layout of the reference's nn/nets.py and nn/net_blocks.py, so `getattr(nets, config['NN']['model'])`
(nn/train.py:120) resolves against this package unchanged.  All arithmetic runs in libgpe_hip.so
(include/gpe_hip.h); see DESIGN.md.

`ops` is the host side of the kernels and the one name callers use: the training hot path and every switch that callers rebind
live in ops.py; the stitch classifier, the losses, the data samplers and the evaluation live in ops_stitch / ops_losses / ops_data /
ops_eval on top of _opbase and are re-exported by ops.  `ops` is imported before them: ops_stitch needs it complete.

The directory name contains '-', so import it with importlib or through the `gpe_amd` alias module at the
repository root:  `import gpe_amd; from gpe_amd import nets`."""
from . import _lib, streams, _opbase, ops, ops_stitch, ops_losses, ops_data, ops_scan, ops_eval, net_blocks, nets, metrics, optim, parallel, staging, configs, patterns, evaluation  # noqa: F401
from ._lib import set_math, get_math, set_f16x3_min_rows, set_reserved_cus, get_reserved_cus  # noqa: F401

__all__ = ['_lib', 'streams', '_opbase', 'ops', 'ops_stitch', 'ops_losses', 'ops_data', 'ops_scan', 'ops_eval', 'net_blocks', 'nets', 'metrics', 'optim', 'parallel', 'staging', 'configs', 'patterns', 'evaluation', 'set_math', 'get_math', 'set_f16x3_min_rows', 'set_reserved_cus', 'get_reserved_cus']
