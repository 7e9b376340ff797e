"""What tests/test_pack_cpu.py and tests/test_gpu_pack.py share: mz_pack_host's record and tables as numpy (include/mz_engine_debug.h)."""
import ctypes as C

import numpy as np

FIELDS = ('n_flat', 'n_packed', 'w0o', 'b0o', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'w4', 'b4', 'lnw', 'lnb', 'w1f', 'w3f', 'ws', 'h4', 'p4', 'is',
          'wstride', 'n_packed_h2', 'ks0', 'ks1', 'ks3', 'nsteps', 'nst0', 'nroot', 'ngroups')      # MZ_PACK_FIELDS


def pack_host(lib, O, A, Sv, Sr, split, tables=True):
  """-> (record as int64 [29], dict of it, [idx, idx2, idx_h2 or None]; tables False: None for each)"""
  from model_based_rl_amd import _abi
  rec = np.zeros(len(FIELDS), np.int64)
  _abi.check(lib.mz_pack_host(O, A, Sv, Sr, split, rec.ctypes.data, 0, None, 0), 'mz_pack_host')
  p = dict(zip(FIELDS, (int(v) for v in rec)))
  tabs = []
  for which, n in ((0, p['n_packed']), (1, p['n_packed']), (2, p['n_packed_h2'])):
    if not n or not tables:
      tabs.append(None)
      continue
    t = np.empty(n, np.int32)
    _abi.check(lib.mz_pack_host(O, A, Sv, Sr, split, rec.ctypes.data, which, t.ctypes.data, C.c_size_t(n)), 'mz_pack_host')
    tabs.append(t)
  return rec, p, tabs
