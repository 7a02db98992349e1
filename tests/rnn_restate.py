"""The recurrence kernels family by family (csrc/gpe_rnn_seq.hip), restated for the tests: no GPU, no library call.

gpe_rnn_seq_fwd / gpe_rnn_seq_bwd hand a stack to three kernel families in a fixed order (include/gpe_hip.h gpe_rnn_seq_fwd_path /
gpe_rnn_seq_bwd_path name them): 1 persistent with K split over the waves, 2 persistent with waves owning row tiles (forward, fp16
pipe), 3 diagonal launches.  This module holds
  fwd_path / bwd_path   both ladders and every plan number restated from the plan steps of the three families; fwd_ws / bwd_ws the
                        workspace queries.  tests/test_rnn_host.py holds them against the exports on every case and a seeded sweep.
  CASES                 case lists by family and direction; each case names the family it was written for.
  Problem, check_fwd,   the data of a case and the CELL-BY-CELL fp64 checkers: every cell (l, t) is recomputed from what the kernel
  check_bwd             itself produced and consumed, so no error growth over T has to be allowed for; every element is compared on
                        its own against its bar.
  ref_fwd, ref_bwd      the whole sequence in fp64 (held against torch.nn.LSTM / GRU by the host test), for the project's 2e-5 / 1e-4
                        bars on a whole tensor.
  emulate_fwd/_bwd      an fp32 restatement of a family's arithmetic (its K split; the two-term fp16 emulation for the fp16 pipe).
  VARIANTS              wrong references; the checker must reject each on every family that has a case it changes.

THE BARS (derived, not tuned).  u = 2^-24.  A pre-activation z = addend + sum_k w_k a_k is computed by the matrix pipe as chains of
fused multiply-adds that meet in a few more additions; whatever the split, with n operations on the longest path
    |z_dev - z| <= gamma(n) S,  S = |addend| + sum_k |w_k| |a_k|,  gamma(n) = n u / (1 - n u)          (Higham, Accuracy and
Stability, 3.1: holds for every summation order), n = K + 8 for the exact kernels (K products, at most 8 joins of partials and
addends).  On the fp16 pipe each operand enters as two fp16 terms of its value scaled by a power of two that brings the largest
magnitude into [2^14, 2^15) (weights: their amax word; state rows: GPE_STATE_SA = 2^12, |h| < 1): the second term's rounding leaves
|dx| <= 2^-22 |x| + 2^-39 amax (the floor: fp16's subnormal spacing 2^-24, halved, over the scale), and the product of the two
residuals (<= 2^-22 |w| |a|) is dropped: 3 * 2^-22 S + the floors, then 3 K + 8 additions at u.
The activated gate g = act(z): |dg| <= Lip |dz| + m ulp(g), Lip = 1/4 (sigmoid) or 1 (tanh), m = ACT_ULPS ulps of the device's expf /
tanhf.  m is measured ON THE REFERENCE SIDE: the worst difference of torch's CPU fp32 sigmoid / tanh against fp64 over the cases' own
pre-activations, times 4 for a different math library (test_rnn_host.py measures it again and holds it under ACT_ULPS;
profiles/rnn_tests.md).  c_t = f c_{t-1} + i g and h_t = o tanh(c_t) follow by the product rule, each fp32 operation adding u of its
result.  Backward: dh from the returned gate gradients by the same chain bound; the carry (dc_t f_t, GRU: dh_t z_t) is chained in
fp64 along t, its bar accumulating geometrically: e_carry(t) = |f_t| e_dc(t) + u |carry|, e_dc(t) containing e_carry(t + 1)."""
import dataclasses
import math
import zlib

import numpy as np

U = 2.0 ** -24
ACT_ULPS = 8.0              # 4 x the measured 2 ulps (profiles/rnn_tests.md); held by test_rnn_host.py::test_activation_multiple
STATE_SA = 4096.0           # csrc/gpe_device.h GPE_STATE_SA
PS_MAXL = PM_MAXL = 4
PM_FS, PM_NW, PM_MAXQ = 32, 4, 4
PS_LDC, PS_LDB = 68, 20
RG_BM, WV_MAXCELL = 64, 4
LDS_CAP = 160 * 1024
PERSIST, MULTI, DIAG = 1, 2, 3
FAMILY = {PERSIST: 'K-split persistent', MULTI: 'multi-tile persistent', DIAG: 'diagonal launches'}
PLAN_FIELDS = ('f16', 'NB', 'NRT', 'per', 'rgmax', 'RG', 'KP', 'grid', 'lds', 'ws_used', 'ks', 'split', 'jslabs', 'nz', 'fuse', 'Hp',
               'groups')


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


# ------------------------------------------------------------------------------------------------------------------------------
# the ladders and the plan numbers
# ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class State:
    """the process state a plan reads: arithmetic mode, debug word, reserved CUs (without a device: 256 CUs less the reservation)"""
    math: int = 0
    debug: int = 0
    reserved: int = 0
    device_cus: int = 256

    def usable(self, have_device):
        """csrc/gpe_state.hip gpe_num_cus"""
        left = self.device_cus - self.reserved
        return max(left, 8) if have_device else left


def plan_begin(gates, L, maxl, T, Bn, H, off_bits, st, have_device=False):
    if gates != 4 or L < 1 or L > maxl or T < 1 or Bn < 1 or H < 1 or H > 256 or (st.debug & off_bits):
        return None
    NB, NRT, cus = cdiv(H, 16), cdiv(Bn, 16), st.usable(have_device)
    per = L * NB
    if cus <= 0 or per > cus:
        return None
    return dict(NB=NB, NRT=NRT, per=per, rgmax=min(cus // per, NRT))


def ps_plan(gates, L, T, Bn, H, bwd, st, have_device=False):
    pl = plan_begin(gates, L, PS_MAXL, T, Bn, H, 1024, st, have_device)
    if pl is None:
        return None
    pl['RG'] = pl['rgmax']
    if pl['RG'] < pl['NRT'] and not (st.debug & (4096 if bwd else 2048)):
        return None
    pl['grid'] = pl['per'] * pl['RG']
    return pl


def ps_ws_bytes(L, T, pl, st):
    return rup(L * T * pl['NRT'] * 4, 256) + (pl['grid'] * T * 64 if st.debug & 8192 else 0)


def pm_plan(gates, L, T, Bn, H, st, have_device=False):
    pl = plan_begin(gates, L, PM_MAXL, T, Bn, H, 1024 | 131072, st, have_device)
    if pl is None:
        return None
    pl['KP'] = rup(H, 32)
    if pl['KP'] != 16 * pl['NB']:
        return None

    def crit(rg):
        return cdiv(cdiv(pl['NRT'], rg), 4)
    pl['RG'] = min(rg for rg in range(1, pl['rgmax'] + 1) if crit(rg) <= crit(pl['rgmax']))
    pl['grid'] = pl['per'] * pl['RG']
    return pl


def pm_ws_bytes(L, T, pl, st):
    return (L * (T + 1) * pl['NRT'] * PM_FS * 4 + L * (T + 1) * 16 * pl['NRT'] * pl['KP'] * 4 +
            (pl['grid'] * PM_NW * T * PM_MAXQ * 64 if st.debug & 8192 else 0))


def _dims_ok(gates, L, T, Bn, H):
    return gates in (3, 4) and L > 0 and T > 0 and Bn > 0 and H > 0


def fwd_ws(gates, L, T, Bn, H, st, have_device=False):
    """gpe_rnn_seq_fwd_ws"""
    if not _dims_ok(gates, L, T, Bn, H):
        return -22
    a = ps_plan(gates, L, T, Bn, H, False, st, have_device)
    b = pm_plan(gates, L, T, Bn, H, st, have_device)
    return max(ps_ws_bytes(L, T, a, st) if a else 0, pm_ws_bytes(L, T, b, st) if b else 0)


def wave_bwd_ws_floats(gates, L, T, Bn, H):
    nz = cdiv(gates * H, 128)
    return min(L, WV_MAXCELL) * 2 * nz * Bn * rup(H, 4) + (T + L) * WV_MAXCELL * cdiv(Bn, RG_BM) * cdiv(H, 64) + 64


def bwd_ws(gates, L, T, Bn, H, st, have_device=False):
    """gpe_rnn_seq_bwd_ws (floats)"""
    if not _dims_ok(gates, L, T, Bn, H):
        return -22
    a = ps_plan(gates, L, T, Bn, H, True, st, have_device)
    return max(wave_bwd_ws_floats(gates, L, T, Bn, H), (ps_ws_bytes(L, T, a, st) if a else 0) // 4)


def pack_kpad(K):
    """K extent of a plain packed weight (csrc/gpe_pack.hip gpe_pack_kpad)"""
    k16 = rup(K, 16)
    return 160 if 96 < k16 < 160 else 208 if 160 < k16 < 208 else k16


def _fits(ptr, size, need, align):
    return bool(ptr) and size >= need and not (ptr & (align - 1))


def _groups(L, T):
    longest = min(L, T)
    return min(longest, WV_MAXCELL), cdiv(longest, WV_MAXCELL)


def _split_mode(Bn):
    return int(Bn - RG_BM * (cdiv(Bn, RG_BM) - 1) <= 32)


def _plan_out(**kw):
    d = dict.fromkeys(PLAN_FIELDS, 0)
    d.update({k: int(v) for k, v in kw.items()})
    return d


def fwd_path(gates, L, T, Bn, H, hs, hs_sl, hs_sb, hs_st, packs, planes, bias_rows, ws, ws_bytes, st, have_device=False):
    """gpe_rnn_seq_fwd_path restated -> (family or -22, plan dict or None).  hs / ws: the pointers' values"""
    if L < 1 or L > (1 << 20) or packs < 0 or planes < 0:
        return -22, None
    if not _dims_ok(gates, L, T, Bn, H) or not hs or (hs_sb & 3) or (hs_st & 3):
        return -22, None
    f16 = st.math == 4 and planes != 0
    in_use = planes if f16 else packs

    def tables_ok():                       # gpe_rnn_fill_tables: every pack there and 16-byte aligned, the bias rows of layers > 0
        return in_use != 0 and not (in_use & 15) and (L == 1 or bias_rows)
    # 1: persistent, K split over the waves
    pl = ps_plan(gates, L, T, Bn, H, False, st, have_device)
    if pl is not None:
        need = ps_ws_bytes(L, T, pl, st)
        KP = rup(H, 32 if f16 else 16)
        lds = (2 if L > 1 else 1) * KP * 256 + 4 * 16 * PS_LDC * 4
        if (_fits(ws, ws_bytes, need, 8) and Bn * hs_sb * 4 < (1 << 31) and not (hs & 15) and lds <= LDS_CAP and tables_ok()):
            return PERSIST, _plan_out(f16=f16, KP=KP, lds=lds, ws_used=need, **pl)
    # 2: persistent, waves own row tiles
    pl = pm_plan(gates, L, T, Bn, H, st, have_device) if f16 else None
    if pl is not None:
        need = pm_ws_bytes(L, T, pl, st)
        lds = pl['KP'] * 256 + 5 * 16384
        if L > 1:
            lds = max(lds, 2 * pl['KP'] * 256 + 16384 + 256)
        if (_fits(ws, ws_bytes, need, 16) and 16 * pl['NRT'] * pl['KP'] * 4 < (1 << 31) and not (hs_sl & 3) and not (hs & 15) and
                lds <= LDS_CAP and cdiv(cdiv(pl['NRT'], pl['RG']), PM_NW) <= PM_MAXQ and tables_ok()):
            return MULTI, _plan_out(f16=1, lds=lds, ws_used=need, **pl)
    # 3: the diagonals
    ks = 256 if Bn <= RG_BM else 128
    kp = rup(min(H, ks), 32 if f16 else 16)
    lds = (RG_BM * max(kp + 4, 32 * gates + 4) + kp * 16 * gates) * 4
    if lds > LDS_CAP:
        return -22, None
    cells, groups = _groups(L, T)
    return DIAG, _plan_out(f16=f16, KP=kp, lds=lds, ks=ks, split=_split_mode(Bn), grid=cdiv(Bn, RG_BM) * cdiv(H, 16) * cells,
                           groups=groups)


def bwd_path(gates, L, T, Bn, H, dgx, dg_sl, dg_sb, dg_st, part, packs, planes, st, have_device=False):
    """gpe_rnn_seq_bwd_path restated"""
    if L < 1 or L > (1 << 20) or packs < 0 or planes < 0:
        return -22, None
    if not _dims_ok(gates, L, T, Bn, H) or not dgx or not part or (dg_sb & 3) or (dg_st & 3):
        return -22, None
    f16 = st.math == 4 and planes != 0
    in_use = planes if f16 else packs
    pl = ps_plan(gates, L, T, Bn, H, True, st, have_device)
    if pl is not None:
        need = ps_ws_bytes(L, T, pl, st)
        K = 4 * H
        KP = rup(K, 32) if f16 else pack_kpad(K)
        lds = (2 if L > 1 else 1) * KP * 64 + 4 * 16 * PS_LDB * 4
        if (not (part & 7) and Bn * dg_sb * 4 < (1 << 31) and not (dgx & 15) and not (dg_sl & 3) and K <= KP <= 1024 and
                not (KP & (31 if f16 else 15)) and lds <= LDS_CAP and in_use != 0 and not (in_use & 15)):
            return PERSIST, _plan_out(f16=f16, KP=KP, lds=lds, ws_used=need // 4, **pl)
    K, KS = gates * H, 128
    jslabs = min(cdiv(K, KS), 4) if Bn > 3 * RG_BM else 1
    nz = cdiv(cdiv(K, KS), jslabs)
    fuse = int(gates == 4 and L <= WV_MAXCELL and bool(st.debug & 65536))
    Hp = rup(H, 4) if fuse else H
    gx, gy, ncell = cdiv(Bn, RG_BM), cdiv(H, 64), min(L, WV_MAXCELL)
    images = ncell * 2 * nz * Bn * Hp
    cells, groups = _groups(L, T)
    used = rup(images, 16) + (T + L) * WV_MAXCELL * gx * gy if fuse else images
    return DIAG, _plan_out(ks=KS, split=_split_mode(Bn), jslabs=jslabs, nz=nz, fuse=fuse, Hp=Hp, groups=groups,
                           lds=(RG_BM * (KS + 4) + KS * 64) * 4, grid=gx * gy * cells * 2 * nz, ws_used=used)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """one call.  family: what the case was written for; reserved / math / debug: the process state it runs under.  why: the refusal
    or boundary it is there for.  Layout switches (GPU run and path query alike): strided = gaps between rows, slots and layers of every
    tensor; seq = a layer-0 input per step (xp0_st != 0); hs_off / ws_off / dgx_off / part_off: bytes the base pointer is moved off its
    16-byte alignment; ws: 'ok' / 'short' / 'none'; packs / planes / bias_rows as the exports take them; hs_sl_odd: a layer stride of hs
    that is no multiple of 4 floats; no_dtop / no_dhN / no_dcN: that gradient is absent.  gpu: the case is launched (a case whose
    operand tables are incomplete or misaligned is asked of the plan only: the diagonals would follow the missing pointer)"""
    family: int
    gates: int
    L: int
    T: int
    Bn: int
    H: int
    reserved: int = 0
    math: int = 0
    debug: int = 0
    why: str = ''
    strided: bool = False
    seq: bool = False
    hs_off: int = 0
    ws_off: int = 0
    ws: str = 'ok'
    dgx_off: int = 0
    part_off: int = 0
    hs_sl_odd: bool = False
    dg_sl_odd: bool = False
    packs: int = 16
    planes: int = 16
    bias_rows: int = 1
    no_dtop: bool = False
    no_dhN: bool = False
    no_dcN: bool = False
    gpu: bool = True

    @property
    def state(self):
        return State(self.math, self.debug, self.reserved)

    @property
    def f16(self):
        return self.math == 4 and self.planes != 0


def case_id(c):
    kind = 'lstm' if c.gates == 4 else 'gru'
    s = '%s-L%dT%dB%dH%d-r%d-m%d' % (kind, c.L, c.T, c.Bn, c.H, c.reserved, c.math)
    if c.debug:
        s += '-d%d' % c.debug
    return s + ('-' + c.why.replace(' ', '_') if c.why else '')


def _C(family, L, T, Bn, H, **kw):
    kw.setdefault('gates', 4)
    return Case(family=family, L=L, T=T, Bn=Bn, H=H, **kw)


R64 = 192                   # reservation that leaves 64 usable CUs, the fewest (gpe_reserve_cus_set)

CASES = {
    # ---- forward -----------------------------------------------------------------------------------------------------------------
    'persist_fwd': [
        _C(PERSIST, 2, 1, 5, 20, why='one step ragged tile'),
        _C(PERSIST, 2, 3, 16, 20, why='whole tile'),
        _C(PERSIST, 2, 3, 17, 20, strided=True, why='two tiles strided'),
        _C(PERSIST, 2, 3, 33, 20, math=4, why='fp16 pipe three tiles'),
        _C(PERSIST, 1, 3, 20, 16, seq=True, why='one layer sequence input'),
        _C(PERSIST, 2, 2, 9, 17, why='ragged unit block'),
        _C(PERSIST, 1, 2, 16, 256, why='most units'),
        _C(PERSIST, 4, 3, 7, 20, why='most layers'),
        _C(PERSIST, 4, 3, 7, 20, math=4, planes=0, why='tables incomplete exact bits'),
        _C(PERSIST, 4, 2, 80, 64, reserved=R64, debug=2048, why='several row tiles per workgroup'),
        _C(PERSIST, 4, 2, 80, 64, reserved=R64, debug=2048, math=4, strided=True, why='several row tiles fp16 strided'),
        _C(PERSIST, 2, 3, 1, 1, why='one unit one row'),
    ],
    'multi_fwd': [
        _C(MULTI, 4, 3, 80, 64, reserved=R64, math=4, why='rgmax 4 of 5 tiles'),
        _C(MULTI, 4, 3, 309, 64, reserved=R64, math=4, strided=True, why='seven tiles ragged last'),
        _C(MULTI, 1, 3, 260, 50, reserved=R64, math=4, seq=True, why='one layer sequence ragged quad'),
        _C(MULTI, 3, 2, 170, 30, reserved=R64, math=4, seq=True, why='sequence input ragged quad'),
        _C(MULTI, 2, 3, 130, 250, reserved=0, math=4, why='the decoders width'),
    ],
    'diag_fwd': [
        _C(DIAG, 2, 3, 32, 20, gates=3, why='gru split mode'),
        _C(DIAG, 2, 3, 33, 20, gates=3, strided=True, why='gru no split strided'),
        _C(DIAG, 2, 3, 33, 20, gates=3, math=4, why='gru fp16 pipe'),
        _C(DIAG, 2, 2, 65, 130, gates=3, math=4, seq=True, why='gru fp16 pipe narrow slab 128 plus 2'),
        _C(DIAG, 2, 3, 32, 20, debug=1024, why='lstm split mode'),
        _C(DIAG, 2, 3, 33, 20, debug=1024, why='lstm no split'),
        _C(DIAG, 2, 2, 64, 40, debug=1024, math=4, why='wide slab fp16'),
        _C(DIAG, 2, 2, 65, 130, debug=1024, why='narrow slab 128 plus 2'),
        _C(DIAG, 2, 2, 65, 130, debug=1024, math=4, strided=True, why='narrow slab fp16 strided'),
        _C(DIAG, 1, 2, 20, 260, why='wide slab 256 plus 4'),
        _C(DIAG, 1, 2, 20, 260, gates=3, seq=True, why='gru wide slab 256 plus 4'),
        _C(DIAG, 5, 3, 17, 20, why='five layers groups 4 plus 1'),
        _C(DIAG, 6, 6, 9, 17, gates=3, why='six layers groups 4 plus 2'),
        _C(DIAG, 3, 2, 20, 20, debug=1024, seq=True, why='fewer steps than layers'),
        _C(DIAG, 2, 1, 5, 1, gates=3, why='one unit one step'),
        # ---- every refusal of the persistent families, alone: the same stack runs there without it
        _C(DIAG, 2, 3, 17, 20, debug=1024, why='refused bit 1024'),
        _C(DIAG, 2, 3, 17, 257, why='refused more than 256 units'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, why='refused row tiles outnumber the row groups'),
        _C(DIAG, 2, 3, 17, 20, ws='none', why='refused no workspace'),
        _C(DIAG, 2, 3, 17, 20, ws='short', why='refused short workspace'),
        _C(DIAG, 2, 3, 17, 20, ws_off=4, why='refused workspace not 8 byte aligned'),
        _C(DIAG, 2, 3, 17, 20, hs_off=4, gpu=False, why='refused hs not 16 byte aligned'),
        _C(DIAG, 2, 3, 17, 20, packs=8, gpu=False, why='refused pack misaligned'),
        _C(DIAG, 2, 3, 17, 20, packs=0, gpu=False, why='refused pack missing'),
        _C(DIAG, 2, 3, 17, 20, bias_rows=0, gpu=False, why='refused bias row missing'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, math=4, debug=131072, why='multi tile refused bit 131072'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, math=4, planes=0, why='multi tile refused not f16'),
        _C(DIAG, 4, 2, 100, 40, reserved=R64, math=4, why='multi tile refused KP is not 16 NB'),
        _C(DIAG, 4, 2, 1025, 64, reserved=R64, math=4, why='multi tile refused more than PM_MAXQ tiles a wave'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, math=4, ws_off=8, why='multi tile refused workspace not 16 byte aligned'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, math=4, hs_sl_odd=True, gpu=False, why='multi tile refused layer stride not in quads'),
        _C(DIAG, 5, 2, 80, 64, reserved=R64, math=4, why='multi tile refused five layers'),
    ],
    # ---- backward ----------------------------------------------------------------------------------------------------------------
    'persist_bwd': [
        _C(PERSIST, 2, 1, 5, 20, why='one step ragged tile'),
        _C(PERSIST, 2, 3, 17, 20, strided=True, why='two tiles strided'),
        _C(PERSIST, 2, 3, 33, 20, math=4, why='fp16 pipe'),
        _C(PERSIST, 2, 2, 9, 17, no_dtop=True, why='ragged unit block no dtop'),
        _C(PERSIST, 1, 2, 16, 256, no_dhN=True, why='most units no dhN'),
        _C(PERSIST, 4, 3, 7, 20, no_dcN=True, why='most layers no dcN'),
        _C(PERSIST, 2, 3, 16, 20, no_dhN=True, no_dcN=True, why='dtop only'),
        _C(PERSIST, 2, 2, 20, 16, why='whole unit block'),
        _C(PERSIST, 2, 3, 17, 20, math=4, planes=0, why='tables incomplete exact bits'),
        _C(PERSIST, 4, 2, 80, 64, reserved=R64, debug=4096, math=4, planes=0, why='several row tiles tables incomplete exact bits'),
        _C(PERSIST, 4, 2, 80, 64, reserved=R64, debug=4096, why='several row tiles per workgroup'),
        _C(PERSIST, 4, 2, 80, 64, reserved=R64, debug=4096, math=4, strided=True, why='several row tiles fp16 strided'),
    ],
    'diag_bwd': [
        _C(DIAG, 2, 3, 32, 20, gates=3, why='gru split mode'),
        _C(DIAG, 2, 3, 33, 20, gates=3, strided=True, no_dhN=True, why='gru strided no dhN'),
        _C(DIAG, 2, 2, 192, 40, debug=1024, why='one slab per workgroup'),
        _C(DIAG, 2, 2, 193, 40, debug=1024, why='two slabs per workgroup'),
        _C(DIAG, 2, 2, 193, 130, debug=1024, strided=True, why='four slabs of five'),
        _C(DIAG, 2, 3, 17, 20, debug=1024 | 65536, why='fused'),
        _C(DIAG, 4, 2, 70, 66, debug=1024 | 65536, strided=True, why='fused ragged quad two column blocks'),
        _C(DIAG, 5, 3, 17, 20, debug=65536, why='five layers not fused'),
        _C(DIAG, 6, 6, 9, 17, gates=3, no_dtop=True, why='six layers no dtop'),
        _C(DIAG, 3, 2, 20, 20, debug=1024, no_dcN=True, why='fewer steps than layers no dcN'),
        _C(DIAG, 2, 3, 17, 20, debug=1024, no_dtop=True, no_dhN=True, why='dcN only'),
        _C(DIAG, 2, 3, 17, 20, debug=1024, no_dtop=True, no_dcN=True, why='dhN only'),
        _C(DIAG, 2, 3, 17, 20, debug=1024, math=4, planes=0, why='tables incomplete exact bits'),
        _C(DIAG, 2, 3, 17, 20, debug=1024, math=4, why='fp16 mode the diagonals stay exact'),
        # ---- every refusal of the persistent family, alone
        _C(DIAG, 2, 3, 17, 257, why='refused more than 256 units'),
        _C(DIAG, 4, 2, 80, 64, reserved=R64, why='refused row tiles outnumber the row groups'),
        _C(DIAG, 2, 3, 17, 20, part_off=4, why='refused workspace not 8 byte aligned'),
        _C(DIAG, 2, 3, 17, 20, dgx_off=8, gpu=False, why='refused dgx not 16 byte aligned'),
        _C(DIAG, 2, 3, 17, 20, dg_sl_odd=True, gpu=False, why='refused layer stride of dgx not in quads'),
        _C(DIAG, 5, 2, 17, 20, why='refused five layers'),
        _C(DIAG, 2, 3, 17, 20, packs=8, gpu=False, why='refused pack misaligned'),
        _C(DIAG, 2, 3, 17, 20, packs=0, gpu=False, why='refused pack missing'),
    ],
}
# Refusals of DESIGN.md 5.28 without a case, because no call reaches them alone: "L NB workgroups exceed the usable CUs" (L <= 4 and
# NB <= 16 give at most 64, the fewest usable CUs); "LDS above 160 KB" and the backward's KP checks (H <= 256 keeps every image below
# 148 KB and KP = 4H rounded up to a k-step at most 1024); "a row image >= 2 GiB" (exempt: more than 2 GiB); "row pitch not in quads"
# (the entry points refuse it for every family).  hs / dgx off their 16-byte alignment, a layer stride of hs outside quads and
# incomplete operand tables are asked of the plan only (gpu=False): the diagonals fetch rows in 16-byte pieces and follow every pointer.
FORWARD = ('persist_fwd', 'multi_fwd', 'diag_fwd')
BACKWARD = ('persist_bwd', 'diag_bwd')
# the family whose forward makes a backward group's history: its own, the diagonals' where it has none
HISTORY_OF = {'persist_bwd': PERSIST, 'diag_bwd': DIAG}


def gpu_cases(group):
    return [c for c in CASES[group] if c.gpu]


# ---- the layout of a case's buffers (floats), shared by the path query on stand-in pointers and by the GPU run
def layout(c):
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    gap = 4 if c.strided else 0
    Hp = rup(H, 4) + gap                                  # slot pitch of a state row: its pad columns
    hs_sb = (T + 1) * Hp + gap
    hs_sl = Bn * hs_sb + gap + (2 if c.hs_sl_odd else 0)
    cs_st = Bn * H + (3 if c.strided else 0)
    cs_sl = (T + 1) * cs_st + (5 if c.strided else 0)
    sv_st = Bn * 4 * H + (3 if c.strided else 0)
    sv_sl = T * sv_st + (5 if c.strided else 0)
    GHp = rup(G * H, 4) + gap
    dg_sb = T * GHp + gap
    dg_sl = Bn * dg_sb + gap + (2 if c.dg_sl_odd else 0)
    xw = G * H + (3 if c.strided else 0)
    xp0_st = xw if c.seq else 0
    xp0_sb = (T if c.seq else 1) * xw + (2 if c.strided else 0)
    dt_st = H + (3 if c.strided else 0)
    dt_sb = T * dt_st + (2 if c.strided else 0)
    return dict(Hp=Hp, hs_sb=hs_sb, hs_sl=hs_sl, hs_st=Hp, cs_st=cs_st, cs_sl=cs_sl, sv_st=sv_st, sv_sl=sv_sl, GHp=GHp, dg_st=GHp,
                dg_sb=dg_sb, dg_sl=dg_sl, xp0_sb=xp0_sb, xp0_st=xp0_st, dt_sb=dt_sb, dt_st=dt_st,
                hs_n=L * hs_sl, cs_n=L * cs_sl, sv_n=L * sv_sl, dg_n=L * dg_sl, xp_n=Bn * xp0_sb, dt_n=Bn * dt_sb)


def ws_bytes_given(c, have_device=False):
    """the bytes of forward workspace the case hands over"""
    need = fwd_ws(c.gates, c.L, c.T, c.Bn, c.H, c.state, have_device)
    if c.ws == 'short':                    # four bytes less than the smaller of the two persistent layouts
        a = ps_plan(c.gates, c.L, c.T, c.Bn, c.H, False, c.state, have_device)
        b = pm_plan(c.gates, c.L, c.T, c.Bn, c.H, c.state, have_device)
        sizes = [n for n in (ps_ws_bytes(c.L, c.T, a, c.state) if a else 0, pm_ws_bytes(c.L, c.T, b, c.state) if b else 0) if n]
        return min(sizes) - 4 if sizes else 0
    return 0 if c.ws == 'none' else need


def fwd_path_args(c, hs_ptr, ws_ptr, have_device=False):
    """gpe_rnn_seq_fwd_path's arguments without plan_out; hs_ptr / ws_ptr: 64-byte aligned addresses the case's offsets are added to"""
    lay = layout(c)
    nbytes = ws_bytes_given(c, have_device)
    return (c.gates, c.L, c.T, c.Bn, c.H, hs_ptr + c.hs_off, lay['hs_sl'], lay['hs_sb'], lay['hs_st'], c.packs, c.planes, c.bias_rows,
            0 if c.ws == 'none' else ws_ptr + c.ws_off, nbytes)


def bwd_path_args(c, dgx_ptr, part_ptr):
    lay = layout(c)
    return (c.gates, c.L, c.T, c.Bn, c.H, dgx_ptr + c.dgx_off, lay['dg_sl'], lay['dg_sb'], lay['dg_st'], part_ptr + c.part_off, c.packs,
            c.planes)


# ------------------------------------------------------------------------------------------------------------------------------
# data, whole-sequence references
# ------------------------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


@dataclasses.dataclass
class Problem:
    """the data of a case, fp32 values held in fp64 arrays where the references read them.  w_ih[0] is layer 0's input weight [G H, In]
    (the kernels see only xproj0 = x W_ih0^T + b, rounded to fp32); bias[l]: the addend row of layer l as the entry point takes it
    (LSTM b_ih + b_hh; GRU b_ih + [b_hr | b_hz | 0]); bhn: GRU b_hn"""
    case: Case
    w_ih: list
    w_hh: list
    b_ih: list
    b_hh: list
    bias: list
    bhn: list
    x: np.ndarray
    xproj0: np.ndarray          # [Bn, T, G H] (a constant input repeated)
    h0: np.ndarray
    c0: np.ndarray
    dtop: object
    d_hN: object
    d_cN: object


def f32(a):
    return np.asarray(a, dtype=np.float32)


def make_problem(c, integer=False):
    """seeded by the case.  integer: small-integer weights and states (every summation order is exact)"""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    In = 6

    def draw(*shape, scale=1.0):
        if integer:
            return rng.integers(-2, 3, size=shape).astype(np.float64)
        return f32(rng.uniform(-1, 1, size=shape) * scale).astype(np.float64)
    k = 1.0 if integer else 1.5 / math.sqrt(H)          # torch's 1 / sqrt(H) init, a little livelier
    w_ih = [draw(G * H, In if l == 0 else H, scale=k) for l in range(L)]
    w_hh = [draw(G * H, H, scale=k) for l in range(L)]
    b_ih = [draw(G * H, scale=0.5) for l in range(L)]
    b_hh = [draw(G * H, scale=0.5) for l in range(L)]
    bias, bhn = [], []
    for l in range(L):
        if G == 4:
            bias.append(f32(b_ih[l] + b_hh[l]).astype(np.float64))
            bhn.append(None)
        else:
            b = b_ih[l].copy()
            b[:2 * H] += b_hh[l][:2 * H]
            bias.append(f32(b).astype(np.float64))
            bhn.append(b_hh[l][2 * H:].copy())
    x = draw(Bn, T if c.seq else 1, In)
    xproj0 = f32(x @ w_ih[0].T + bias[0]).astype(np.float64)
    xproj0 = np.broadcast_to(xproj0, (Bn, T, G * H)).copy()
    h0 = draw(L, Bn, H, scale=0.9)
    c0 = draw(L, Bn, H, scale=1.5)
    dtop = None if c.no_dtop else draw(Bn, T, H)
    d_hN = None if c.no_dhN else draw(L, Bn, H)
    d_cN = None if (c.no_dcN or G == 3) else draw(L, Bn, H)
    return Problem(c, w_ih, w_hh, b_ih, b_hh, bias, bhn, x, xproj0, h0, c0, dtop, d_hN, d_cN)


def _cell_pre(p, l, t, h_rec, h_below, variant=None):
    """pre-activations of cell (l, t) in fp64 -> (zx, zh, S): input-side part incl. the addend, recurrent part, and the sum of
    magnitudes the chain bound takes.  variant: a wrong reference (VARIANTS)"""
    c = p.case
    H, G, L = c.H, c.gates, c.L
    if l == 0:
        add = p.xproj0[:, t]
        zx, Sx = add.copy(), np.abs(add)
    else:
        wl = l
        if variant == 'wih_wrong_layer':
            wl = l - 1 if l >= 2 else l + 1
        add = np.zeros_like(p.bias[l]) if variant == 'bias_dropped' else p.bias[l]
        zx = add + h_below @ p.w_ih[wl].T
        Sx = np.abs(add) + np.abs(h_below) @ np.abs(p.w_ih[wl]).T
    zh = h_rec @ p.w_hh[l].T
    Sh = np.abs(h_rec) @ np.abs(p.w_hh[l]).T
    return zx, zh, Sx + Sh


def _swap(z, H, variant):
    if variant == 'gates_swapped':
        z = z.copy()
        z[:, :H], z[:, H:2 * H] = z[:, H:2 * H].copy(), z[:, :H].copy()
    return z


def _cell_fwd(p, l, zx, zh, c_prev, h_prev, variant=None):
    """fp64 cell from pre-activations -> (saved [Bn, 4H], c_new or None, h_new)"""
    H = p.case.H
    if p.case.gates == 4:
        z = _swap(zx + zh, H, variant)
        i, f, g, o = sigmoid(z[:, :H]), sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), sigmoid(z[:, 3 * H:])
        cn = f * c_prev + i * g
        return np.concatenate([i, f, g, o], 1), cn, o * np.tanh(cn)
    zx, zh = _swap(zx, H, variant), _swap(zh, H, variant)
    r, z = sigmoid(zx[:, :H] + zh[:, :H]), sigmoid(zx[:, H:2 * H] + zh[:, H:2 * H])
    if variant == 'bhn_outside':
        hn = zh[:, 2 * H:]
        n = np.tanh(zx[:, 2 * H:] + r * hn + p.bhn[l])
        hn = hn + p.bhn[l]
    else:
        hn = zh[:, 2 * H:] + p.bhn[l]
        n = np.tanh(zx[:, 2 * H:] + r * hn)
    return np.concatenate([r, z, n, hn], 1), None, (1 - z) * n + z * h_prev


def ref_fwd(p):
    """the whole sequence in fp64 -> hs [L, Bn, T + 1, H], cs [L, T + 1, Bn, H] (GRU: None), saved [L, T, Bn, 4H]"""
    c = p.case
    L, T, Bn, H = c.L, c.T, c.Bn, c.H
    hs = np.zeros((L, Bn, T + 1, H))
    cs = np.zeros((L, T + 1, Bn, H)) if c.gates == 4 else None
    saved = np.zeros((L, T, Bn, 4 * H))
    hs[:, :, 0] = p.h0
    if cs is not None:
        cs[:, 0] = p.c0
    for t in range(T):
        for l in range(L):
            zx, zh, _ = _cell_pre(p, l, t, hs[l, :, t], hs[l - 1, :, t + 1] if l else None)
            sv, cn, hn = _cell_fwd(p, l, zx, zh, cs[l, t] if cs is not None else None, hs[l, :, t])
            saved[l, t], hs[l, :, t + 1] = sv, hn
            if cs is not None:
                cs[l, t + 1] = cn
    return dict(hs=hs, cs=cs, saved=saved)


def ref_bwd(p, fwd):
    """the whole backward in fp64 from a forward history (arrays as ref_fwd returns them) -> dgx, dgh [L, Bn, T, G H], carry0 [L, Bn, H]"""
    c = p.case
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    dgx = np.zeros((L, Bn, T, G * H))
    dgh = np.zeros((L, Bn, T, G * H))
    carry = np.zeros((L, Bn, H))
    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            dh = np.zeros((Bn, H))
            if l == L - 1 and p.dtop is not None:
                dh = dh + p.dtop[:, t]
            if t == T - 1 and p.d_hN is not None:
                dh = dh + p.d_hN[l]
            if t < T - 1:
                dh = dh + dgh[l, :, t + 1] @ p.w_hh[l]
            if l < L - 1:
                dh = dh + dgx[l + 1, :, t] @ p.w_ih[l + 1]
            cin = carry[l] if t < T - 1 else (p.d_cN[l] if (G == 4 and p.d_cN is not None) else np.zeros((Bn, H)))
            gx, gh, cout = _cell_bwd(p, fwd, l, t, dh, cin)
            dgx[l, :, t], dgh[l, :, t], carry[l] = gx, gh, cout
    return dict(dgx=dgx, dgh=dgh, carry0=carry)


def _cell_bwd(p, fwd, l, t, dh, cin):
    """fp64 pointwise backward of cell (l, t): dh without the carry, cin the carry -> (gx, gh, carry_out)"""
    H = p.case.H
    sv = fwd['saved'][l, t]
    if p.case.gates == 4:
        i, f, g, o = sv[:, :H], sv[:, H:2 * H], sv[:, 2 * H:3 * H], sv[:, 3 * H:]
        ct, cp = fwd['cs'][l, t + 1], fwd['cs'][l, t]
        tc = np.tanh(ct)
        dc = dh * o * (1 - tc * tc) + cin
        gx = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        return gx, gx, dc * f
    r, z, n, hn = sv[:, :H], sv[:, H:2 * H], sv[:, 2 * H:3 * H], sv[:, 3 * H:]
    hp = fwd['hs'][l, :, t]
    dh = dh + cin
    dn = dh * (1 - z) * (1 - n * n)
    dz = dh * (hp - n) * z * (1 - z)
    dr = dn * hn * r * (1 - r)
    return np.concatenate([dr, dz, dn], 1), np.concatenate([dr, dz, dn * r], 1), dh * z


# ------------------------------------------------------------------------------------------------------------------------------
# bars and the cell-by-cell checkers
# ------------------------------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1 - n * U)


def ulp(v):
    """one fp32 unit in the last place of |v| (of the smallest normal number below it)"""
    a = np.maximum(np.abs(v), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def pre_bar(S, K, f16, amax_w=0.0, amax_a=1.0, sum_w=0.0, sum_a=0.0):
    """|z_dev - z| for a chain over K products with magnitude sum S (module docstring).  f16: amax_w / amax_a the largest magnitudes
    the operands' scales come from (state rows: 2^14 / GPE_STATE_SA = 4), sum_w / sum_a the sums of |w| / |a| over the chain"""
    if not f16:
        return gamma(K + 8) * S
    return (3 * 2.0 ** -22 + gamma(3 * K + 8)) * S + 2.0 ** -39 * (amax_a * sum_w + amax_w * sum_a)


def _act_bar(ez, val, lip):
    return lip * ez + ACT_ULPS * ulp(val)


class Worst:
    """collects |got - want| / bar over every element of every tensor; nothing is filtered"""

    def __init__(self):
        self.fig = {}
        self.where = {}
        self.cells = {}                 # (tensor, cell) -> (got, want, bar): what `agree` compares two runs by

    def add(self, name, got, want, bar, at, keep=True):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape == bar.shape, (name, got.shape, want.shape, bar.shape)
        if keep:
            self.cells[name, at] = (got, want, bar)
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.abs(got - want) / bar
        r = np.where(np.isfinite(got), r, np.inf)
        r = np.where((got == want), 0.0, r)                 # (a zero bar on an exact value)
        m = float(r.max()) if r.size else 0.0
        if m >= self.fig.get(name, -1.0):
            self.fig[name] = m
            self.where[name] = at + tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape)) if r.size else at

    @property
    def worst(self):
        return max(self.fig.values()) if self.fig else 0.0

    def __str__(self):
        return ', '.join('%s %.3g bars at %s' % (k, v, self.where[k]) for k, v in sorted(self.fig.items()))


def agree(wa, wb):
    """Two runs of one case by different families (the Worst records of their cell-by-cell checks), element by element: every output
    element of every cell of run A against run B's within the SUM OF THE TWO PER-CELL BARS, plus what the difference of the rows the
    two cells consumed propagates to that element.  The propagated part is not estimated by a Lipschitz constant: each record holds
    the fp64 cell applied to its own run's consumed rows, so |want_A - want_B| is that difference exactly.  It is exactly zero where
    both cells consumed identical rows (cell (0, 0); every cell of a backward pair, up to the gate gradients already returned),
    and there the comparison is within the sum of the bars alone -> Worst"""
    assert set(wa.cells) == set(wb.cells)
    w = Worst()
    for (name, at), (ga, ra, ba) in wa.cells.items():
        gb, rb, bb = wb.cells[name, at]
        w.add(name, ga, gb, ba + bb + np.abs(ra - rb), at, keep=False)
    return w


def check_fwd(p, out, f16=None, variant=None):
    """every cell recomputed in fp64 from the returned history -> Worst.  out: hs [L, Bn, T + 1, H], cs [L, T + 1, Bn, H], saved
    [L, T, Bn, 4H] as the device returned them (fp32)"""
    c = p.case
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    f16 = c.f16 if f16 is None else f16
    hs, saved = out['hs'].astype(np.float64), out['saved']
    cs = out['cs'].astype(np.float64) if G == 4 else None
    w = Worst()
    for l in range(L):
        K = H if l == 0 else 2 * H
        aw = max(float(np.abs(p.w_hh[l]).max()), float(np.abs(p.w_ih[l]).max()) if l else 0.0)
        sum_w = np.abs(p.w_hh[l]).sum(1) + (np.abs(p.w_ih[l]).sum(1) if l else 0.0)
        for t in range(T):
            slot = t + 1 if variant == 'hs_slot_off' else t
            h_rec = hs[l, :, slot]
            h_below = hs[l - 1, :, t + 1] if l else None
            zx, zh, S = _cell_pre(p, l, t, h_rec, h_below, variant)
            sum_a = np.abs(h_rec).sum(1, keepdims=True) + (np.abs(h_below).sum(1, keepdims=True) if l else 0.0)
            # (the state rows' scale is fixed: the floor of their second term is 2^-25 / GPE_STATE_SA = 2^-39 x 4)
            ez = pre_bar(S, K, f16, aw, 4.0, sum_w[None, :], sum_a) + 2 * U * np.abs(zx + zh)
            cp = None
            if G == 4:
                cp = cs[l, t + 1] if variant == 'c_t_for_c_prev' else cs[l, t]
            sv, cn, hn = _cell_fwd(p, l, zx, zh, cp, hs[l, :, t], variant)
            if variant == 'ragged_unit_zeroed':
                sv = sv.copy()
                hn = hn.copy()
                for q in range(4):
                    sv[:, q * H + H - 1] = 0
                hn[:, H - 1] = 0
            if variant == 'ragged_row_neighbour':
                sv, hn = sv.copy(), hn.copy()
                sv[Bn - 1], hn[Bn - 1] = sv[Bn - 2], hn[Bn - 2]
            if G == 4:
                e = [_act_bar(ez[:, q * H:(q + 1) * H], sv[:, q * H:(q + 1) * H], 1.0 if q == 2 else 0.25) for q in range(4)]
                i, f, g, o = (sv[:, q * H:(q + 1) * H] for q in range(4))
                ec = np.abs(cp) * e[1] + np.abs(g) * e[0] + np.abs(i) * e[2] + 3 * U * (np.abs(f * cp) + np.abs(i * g))
                tc = np.tanh(cn)
                eh = np.abs(tc) * e[3] + np.abs(o) * (ec * (1 - tc * tc) + ACT_ULPS * ulp(tc)) + 2 * U * np.abs(hn)
                # (the device forms tanh(c_t) from ITS c_t and o from ITS gate; the returned ones stand in the reference: no more
                # than the terms above, which bound their distance)
                w.add('saved', saved[l, t], sv, np.concatenate(e, 1), (l, t))
                w.add('cs', out['cs'][l, t + 1], cn, ec, (l, t))
                w.add('hs', out['hs'][l, :, t + 1], hn, eh, (l, t))
            else:
                ezx = ez                                           # the two sides share one bound: S covers both chains
                r, z, n, hn_ = (sv[:, q * H:(q + 1) * H] for q in range(4))
                er = _act_bar(ezx[:, :H], r, 0.25)
                ezz = _act_bar(ezx[:, H:2 * H], z, 0.25)
                ehn = ezx[:, 2 * H:] + 2 * U * np.abs(hn_)
                en = _act_bar(ezx[:, 2 * H:] + np.abs(hn_) * er + np.abs(r) * ehn + 3 * U * (np.abs(r * hn_) + np.abs(zx[:, 2 * H:])), n, 1.0)
                hp = hs[l, :, t]
                eh = ezz * (np.abs(n) + np.abs(hp)) + en * np.abs(1 - z) + 4 * U * (np.abs((1 - z) * n) + np.abs(z * hp))
                w.add('saved', saved[l, t], sv, np.concatenate([er, ezz, en, ehn], 1), (l, t))
                w.add('hs', out['hs'][l, :, t + 1], hn, eh, (l, t))
    return w


def check_bwd(p, fwd, out, f16=None, variant=None, carries_out=None):
    """every cell of the backward recomputed in fp64 from the returned gate gradients; only the carry is chained (in fp64, along t
    inside a layer).  fwd: the history the backward ran on (device arrays); out: dgx, dgh [L, Bn, T, G H], carry0 [L, Bn, H]"""
    c = p.case
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    f16 = (c.f16 and c.family == PERSIST) if f16 is None else f16
    F = dict(hs=fwd['hs'].astype(np.float64), saved=fwd['saved'].astype(np.float64),
             cs=fwd['cs'].astype(np.float64) if G == 4 else None)
    dgx, dgh = out['dgx'].astype(np.float64), out['dgh'].astype(np.float64)
    w = Worst()
    K = G * H
    carries = {}
    if variant == 'carry_wrong_layer':                 # the honest chains first: every layer's carry at every step
        check_bwd(p, fwd, out, f16, None, carries)
    for l in range(L - 1, -1, -1):
        carry, ecarry = np.zeros((Bn, H)), np.zeros((Bn, H))
        for t in range(T - 1, -1, -1):
            dh, S, nk = np.zeros((Bn, H)), np.zeros((Bn, H)), 0
            fl = np.zeros((Bn, H))
            if l == L - 1 and p.dtop is not None:
                tt = (t + 1) % T if variant == 'dtop_wrong_step' else t
                dh, S = dh + p.dtop[:, tt], S + np.abs(p.dtop[:, tt])
            if t == T - 1 and p.d_hN is not None and variant != 'dhN_ignored':
                dh, S = dh + p.d_hN[l], S + np.abs(p.d_hN[l])
            for a, wt in ((dgh[l, :, t + 1] if t < T - 1 else None, p.w_hh[l]),
                          (dgx[l + 1, :, t] if l < L - 1 else None, p.w_ih[l + 1] if l < L - 1 else None)):
                if a is None:
                    continue
                dh, S, nk = dh + a @ wt, S + np.abs(a) @ np.abs(wt), nk + K
                if f16:                   # per-wave scales from the largest magnitude loaded: no more than the tensor's
                    fl = fl + 2.0 ** -39 * (float(np.abs(a).max()) * np.abs(wt).sum(0)[None, :] +
                                            float(np.abs(wt).max()) * np.abs(a).sum(1, keepdims=True))
            edh = (pre_bar(S, nk, f16) + fl if nk else 0.0) + 4 * U * S
            if t == T - 1:
                cin = p.d_cN[l] if (G == 4 and p.d_cN is not None and variant != 'dcN_ignored') else np.zeros((Bn, H))
                ecin = np.zeros((Bn, H))
            else:
                cin, ecin = carry, ecarry
                if variant == 'carry_wrong_layer':
                    cin = carries[(l + 1) % L, t + 1]
            gx, gh, cout = _cell_bwd(p, F, l, t, dh, cin)
            sv = F['saved'][l, t]
            if G == 4:
                i, f, g, o = (sv[:, q * H:(q + 1) * H] for q in range(4))
                ct, cp = F['cs'][l, t + 1], F['cs'][l, t]
                tc = np.tanh(ct)
                etc = ACT_ULPS * ulp(tc)
                dc = dh * o * (1 - tc * tc) + cin
                edc = edh * np.abs(o * (1 - tc * tc)) + np.abs(dh * o) * (2 * np.abs(tc) * etc + 3 * U) + ecin + 4 * U * (np.abs(dc) + np.abs(cin))
                ego = edh * np.abs(tc * o * (1 - o)) + np.abs(dh * o * (1 - o)) * etc
                e = np.concatenate([edc * np.abs(g * i * (1 - i)), edc * np.abs(cp * f * (1 - f)), edc * np.abs(i * (1 - g * g)), ego], 1)
                e = e + 6 * U * np.abs(gx)
                ecout = edc * np.abs(f) + U * np.abs(cout)
                w.add('dgx', out['dgx'][l, :, t], gx, e, (l, t))
            else:
                r, z, n, hn = (sv[:, q * H:(q + 1) * H] for q in range(4))
                hp = F['hs'][l, :, t]
                edht = edh + ecin + 2 * U * (np.abs(dh) + np.abs(cin))
                edn = edht * np.abs((1 - z) * (1 - n * n))
                edz = edht * np.abs((hp - n) * z * (1 - z))
                edr = edn * np.abs(hn * r * (1 - r))
                ex = np.concatenate([edr, edz, edn], 1) + 8 * U * np.abs(gx)
                eg = np.concatenate([edr, edz, edn * np.abs(r)], 1) + 8 * U * np.abs(gh)
                ecout = edht * np.abs(z) + U * np.abs(cout)
                w.add('dgx', out['dgx'][l, :, t], gx, ex, (l, t))
                w.add('dgh', out['dgh'][l, :, t], gh, eg, (l, t))
            carry, ecarry = cout, ecout
            if carries_out is not None:
                carries_out[l, t] = cout
        w.add('carry0', out['carry0'][l], carry, ecarry, (l,))
    return w


def whole_seq(got, want):
    """largest difference over largest reference magnitude: the project's bar on a whole tensor"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


SEQ_FWD_BAR, SEQ_BWD_BAR = 2e-5, 1e-4


# ---- wrong references: name -> (direction, does it change this case?)
VARIANTS = {
    'gates_swapped': ('fwd', lambda c: True),
    'bias_dropped': ('fwd', lambda c: c.L > 1),
    'hs_slot_off': ('fwd', lambda c: True),
    'c_t_for_c_prev': ('fwd', lambda c: c.gates == 4),
    'ragged_unit_zeroed': ('fwd', lambda c: c.H % 16 != 0),
    'ragged_row_neighbour': ('fwd', lambda c: c.Bn % 16 != 0 and c.Bn > 1),
    'wih_wrong_layer': ('fwd', lambda c: c.L >= 3),
    'bhn_outside': ('fwd', lambda c: c.gates == 3),
    'dcN_ignored': ('bwd', lambda c: c.gates == 4 and not c.no_dcN),
    'dhN_ignored': ('bwd', lambda c: not c.no_dhN),
    'dtop_wrong_step': ('bwd', lambda c: not c.no_dtop and c.T > 1),
    'carry_wrong_layer': ('bwd', lambda c: c.L > 1 and c.T > 1),
}


# ------------------------------------------------------------------------------------------------------------------------------
# emulate: an fp32 restatement of a family's arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
def _chain32(a, wT, ks, acc=None):
    """fp32 multiply-add chain over the k indices `ks`: acc + sum_k a[:, k] wT[k, :], one rounding per product and per addition"""
    acc = np.zeros((a.shape[0], wT.shape[1]), np.float32) if acc is None else acc
    for k in ks:
        acc = acc + a[:, k:k + 1] * wT[k:k + 1, :]
    return acc


def _split16(v, scale):
    """the two fp16 terms of v * scale (csrc/gpe_device.h gpe_split2_f16), as fp32 arrays"""
    s = f32(v) * np.float32(scale)
    with np.errstate(over='ignore'):       # (columns outside the chain a per-wave scale was taken from; they are not multiplied)
        hi = s.astype(np.float16).astype(np.float32)
        hi = np.where(np.isfinite(hi), hi, np.float32(0))
        lo = (s - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def _scale_of(amax):
    """power of two that brings amax into [2^14, 2^15) (csrc/gpe_common.h gpe_h3_scale_of)"""
    if amax == 0 or not np.isfinite(amax):
        return 1.0
    return 2.0 ** max(-100, min(100, 14 - math.floor(math.log2(amax))))


def _wave_ranges(K, step, waves=4):
    """K split over the waves in whole k-steps (csrc/gpe_rnn_persist.hip: spw = ceil(nsteps / 4))"""
    nsteps = cdiv(K, step)
    spw = cdiv(nsteps, waves)
    return [range(min(w * spw * step, K), min((w + 1) * spw * step, K)) for w in range(waves)]


def _product32(a, w, family, f16, Bn, sa=STATE_SA, dyn=False, ks=128):
    """a [Bn, K] x w [N, K]^T in the family's split, fp32 (or the three-term fp16 product) -> fp32 [Bn, N]"""
    a, wT = f32(a), f32(w).T.copy()
    K = a.shape[1]
    if family == PERSIST:
        parts = _wave_ranges(K, 32 if f16 else 16)
    elif family == MULTI:
        parts = [range(K)]
    else:                                      # slabs of ks in one accumulator; <= 32 rows: two halves of every slab's chunks
        if Bn - RG_BM * (cdiv(Bn, RG_BM) - 1) <= 32 and cdiv(Bn, RG_BM) == 1:
            lo, hi = [], []
            for s0 in range(0, K, ks):
                n = cdiv(min(ks, K - s0), 32 if f16 else 16)
                cut = min(s0 + cdiv(n, 2) * (32 if f16 else 16), K)
                lo += list(range(s0, cut))
                hi += list(range(cut, min(s0 + ks, K)))
            parts = [lo, hi]
        else:
            parts = [range(K)]
    outs = []
    for ksel in parts:
        if not f16:
            outs.append(_chain32(a, wT, ksel))
            continue
        sw = _scale_of(float(np.abs(wT).max()))
        if dyn:
            sa = _scale_of(float(np.abs(a[:, list(ksel)]).max()) if len(ksel) else 0.0)
        ah, al = _split16(a, sa)
        wh, wl = _split16(wT, sw)
        acc = None
        for k in ksel:
            acc = _chain32(al, wh, [k], acc)
            acc = _chain32(ah, wl, [k], acc)
            acc = _chain32(ah, wh, [k], acc)
        acc = np.zeros((a.shape[0], wT.shape[1]), np.float32) if acc is None else acc
        outs.append(acc * np.float32(1.0 / (sw * sa)))
    while len(outs) > 1:
        outs = [outs[i] + outs[i + 1] if i + 1 < len(outs) else outs[i] for i in range(0, len(outs), 2)]
    return outs[0]


def _sig32(x):
    return (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def emulate_fwd(p, family, f16=None):
    """the forward in fp32 as `family` splits it -> arrays like the device's"""
    c = p.case
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    f16 = c.f16 if f16 is None else f16
    ks = 256 if Bn <= RG_BM else 128
    hs = np.zeros((L, Bn, T + 1, H), np.float32)
    cs = np.zeros((L, T + 1, Bn, H), np.float32) if G == 4 else None
    saved = np.zeros((L, T, Bn, 4 * H), np.float32)
    hs[:, :, 0] = p.h0
    if cs is not None:
        cs[:, 0] = p.c0
    for t in range(T):
        for l in range(L):
            zh = _product32(hs[l, :, t], p.w_hh[l], family, f16, Bn, ks=ks)
            add = f32(p.xproj0[:, t]) if l == 0 else f32(p.bias[l])[None, :]
            zx = _product32(hs[l - 1, :, t + 1], p.w_ih[l], family, f16, Bn, ks=ks) if l else None
            if G == 4:
                z = (zh + zx if l else zh) + add
                i, f, g, o = _sig32(z[:, :H]), _sig32(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H], dtype=np.float32), _sig32(z[:, 3 * H:])
                cn = f * cs[l, t] + i * g
                saved[l, t] = np.concatenate([i, f, g, o], 1)
                cs[l, t + 1] = cn
                hs[l, :, t + 1] = o * np.tanh(cn, dtype=np.float32)
            else:
                zx = zx if l else np.zeros_like(zh)
                r = _sig32(zh[:, :H] + zx[:, :H] + add[:, :H])
                z = _sig32(zh[:, H:2 * H] + zx[:, H:2 * H] + add[:, H:2 * H])
                hn = zh[:, 2 * H:] + f32(p.bhn[l])[None, :]
                n = np.tanh(zx[:, 2 * H:] + add[:, 2 * H:] + r * hn, dtype=np.float32)
                saved[l, t] = np.concatenate([r, z, n, hn], 1)
                hs[l, :, t + 1] = (np.float32(1) - z) * n + z * hs[l, :, t]
    return dict(hs=hs, cs=cs, saved=saved)


def emulate_bwd(p, fwd, family, f16=None):
    """the backward in fp32 on the history `fwd` -> dgx, dgh, carry0 like the device's"""
    c = p.case
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    f16 = (c.f16 and family == PERSIST) if f16 is None else f16
    dgx = np.zeros((L, Bn, T, G * H), np.float32)
    dgh = np.zeros((L, Bn, T, G * H), np.float32)
    carry = np.zeros((L, Bn, H), np.float32)
    F = {k: (None if v is None else f32(v)) for k, v in fwd.items()}
    one = np.float32(1)
    for t in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            dh = np.zeros((Bn, H), np.float32)
            if l == L - 1 and p.dtop is not None:
                dh = f32(p.dtop[:, t])
            if t == T - 1 and p.d_hN is not None:
                dh = dh + f32(p.d_hN[l])
            acc = np.zeros((Bn, H), np.float32)
            if l < L - 1:
                acc = acc + _product32(dgx[l + 1, :, t], p.w_ih[l + 1].T, family, f16, Bn, dyn=True)
            if t < T - 1:
                acc = acc + _product32(dgh[l, :, t + 1], p.w_hh[l].T, family, f16, Bn, dyn=True)
            dh = dh + acc
            cin = carry[l] if t < T - 1 else (f32(p.d_cN[l]) if (G == 4 and p.d_cN is not None) else np.zeros((Bn, H), np.float32))
            sv = F['saved'][l, t]
            if G == 4:
                i, f, g, o = (sv[:, q * H:(q + 1) * H] for q in range(4))
                tc = np.tanh(F['cs'][l, t + 1], dtype=np.float32)
                dc = dh * o * (one - tc * tc) + cin
                gx = np.concatenate([dc * g * i * (one - i), dc * F['cs'][l, t] * f * (one - f), dc * i * (one - g * g),
                                     dh * tc * o * (one - o)], 1)
                dgx[l, :, t] = dgh[l, :, t] = gx
                carry[l] = dc * f
            else:
                r, z, n, hn = (sv[:, q * H:(q + 1) * H] for q in range(4))
                dh = dh + cin
                dn = dh * (one - z) * (one - n * n)
                dz = dh * (F['hs'][l, :, t] - n) * z * (one - z)
                dr = dn * hn * r * (one - r)
                dgx[l, :, t] = np.concatenate([dr, dz, dn], 1)
                dgh[l, :, t] = np.concatenate([dr, dz, dn * r], 1)
                carry[l] = dh * z
    return dict(dgx=dgx, dgh=dgh, carry0=carry)


def activation_ulps(pre_sig, pre_tanh):
    """the reference-side measurement behind ACT_ULPS: the worst difference, in fp32 ulps of the value, of torch's CPU fp32 sigmoid /
    tanh against fp64 over the given pre-activations (fp32 arrays) -> (sigmoid, tanh)"""
    import torch
    out = []
    for fn, x in ((torch.sigmoid, pre_sig), (torch.tanh, pre_tanh)):
        x32 = torch.from_numpy(f32(x).ravel().copy())
        got = fn(x32).double().numpy()
        want = fn(x32.double()).numpy()
        out.append(float((np.abs(got - want) / ulp(want)).max()) if got.size else 0.0)
    return tuple(out)
