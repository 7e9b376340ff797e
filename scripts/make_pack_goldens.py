#!/usr/bin/env python3
"""Records tests/golden/pack_sha256.json: the weight streams' gather tables as the engine built them BEFORE csrc/mz_pack.inc existed.

The packing of commit PARENT lives in csrc/mz_engine.hip (FlatLayout, flat_layout .. fill_vec, build_packing_h2, build_packing: the line
ranges below).  It holds no HIP call until its last lines, so it compiles as host C++ once mz_engine, dmalloc, HIPCHECK and hipMemcpy are
stubs and the constants it uses are spelled out (STUBS: values as of PARENT's mz_fused.hip.h, mz_root.hip.h, mz_fused_h2.hip.h).  This tool
reads that text through `git show`, builds it with g++, runs every case and writes per case one SHA-256 each of the offsets record
(pack_plan_record's order, little-endian int64), idx, idx2 and idx_h2 (int32; null without the split-f16 stream).  The only edit to the
parent's text: one line behind `e->n_packed = pos;` that copies seven of build_packing's locals out (they are not visible afterwards).

  python scripts/make_pack_goldens.py            # rewrite the golden file
  python scripts/make_pack_goldens.py --time 50  # seconds per build_packing of the parent (A = 4, O = 8), for the speed comparison
No GPU is touched."""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

PARENT = '76f4bcd'
ENGINE = 'model-based-rl_amd/csrc/mz_engine.hip'
RANGES = ((104, 108), (253, 364), (461, 708))      # FlatLayout; flat_layout .. fill_vec; build_packing_h2, build_packing
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACTIONS = (1, 2, 4, 5, 6, 8, 9, 10, 13, 14, 16, 17, 21, 22, 32)      # both edges of every row of mz_kernels.inc
OBS = (1, 4, 27, 128, 257)
SUPPORTS = ((31, 31), (1, 1), (32, 32), (21, 5))                    # (value bins, reward bins); (1, 1): --no_support
FIELDS = 29


def cases():
  """(obs_dim, action_space, value bins, reward bins, split_f16): the split-f16 stream wherever the kernel covers the action count"""
  return [(o, a, sv, sr, 1 if a <= 13 else 0) for a in ACTIONS for o in OBS for sv, sr in SUPPORTS]


def key(case):
  return 'O%d_A%d_Sv%d_Sr%d_h%d' % case


STUBS = r'''
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <functional>
#include <string>
#include <vector>
#define MZ_H 50
#define MZ_F 512
#define MZ_NB 4
#define MZ_RS_MAIN 13
#define MZ_ATAB_AMAX 4
#define MZ_ATAB_WAVE_FLOATS (MZ_ATAB_AMAX * 256)
static int mz_fused_rs(int ks1, int jtp) { return jtp > 1 ? 9 : (ks1 > 16 ? 11 : (ks1 > 14 ? 12 : MZ_RS_MAIN)); }
static bool mz_fused_atab(int ks1, int jtp, int g) { return ks1 == 14 && jtp == 1 && g == 4; }
static int mz_root_nst0(int O) { return ((O + 1 + 3) / 4 + 1) / 2; }
struct H2Sched { static constexpr int REAL = 25, NGROUPS = 25; };
struct f32x4 { float v[4]; };
struct mz_config { int no_support, value_support_min, value_support_max, reward_support_min, reward_support_max, no_target_transform; };
struct NetView {
  const f32x4 *w0o, *w1, *b1, *w2, *w3, *b3, *w4;
  const float *b0o, *b2, *b4, *lnw, *lnb;
  int ks0, ks1, ks3, O, A, jtp, Sr, Sv, rmin, vmin, no_transform;
};
struct SearchShape { int amax, ks1, jtp, g; };
struct FlatLayout;
static std::string g_err;
static int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}
#define HIPCHECK(x) do { if ((x) != 0) return fail("stub: %s", #x); } while (0)
enum { hipMemcpyHostToDevice = 1 };
static int hipMemcpy(void *dst, const void *src, size_t n, int) { memcpy(dst, src, n); return 0; }
static size_t g_locals[7];
'''

ENGINE_STUB = r'''
struct mz_engine {
  mz_config cfg;
  int A, O, jtp;
  const SearchShape *shape;
  FlatLayout layout;
  size_t n_flat, n_packed, n_packed_h2;
  int32_t *pack_idx, *pack_idx2, *pack_idx_h2;
  float *packed, *relu_scale_dev, *flat_dev;
  unsigned *relu_bound_dev;
  uint16_t *packed_h2;
  NetView nv;
  const f32x4 *wstream, *istream;
  int nst0;
  bool split_f16;
  std::vector<void *> allocs;
};
template <typename T>
static int dmalloc(mz_engine *e, T **p, size_t n) {
  void *q = calloc(n * sizeof(T) + 64, 1);
  e->allocs.push_back(q);
  *p = (T *)q;
  return 0;
}
'''

MAIN = r'''
#define MZ_ROW_F(AMAX, KS1, JTP, G) {AMAX, KS1, JTP, G},
static const SearchShape g_rows[] = {MZ_FUSED_ROWS(MZ_ROW_F)};
static int build(mz_engine &e, int O, int A, int Sv, int Sr, int split) {
  e = mz_engine();
  e.cfg.no_support = Sv == 1 && Sr == 1;
  e.cfg.value_support_min = 0; e.cfg.value_support_max = Sv - 1;
  e.cfg.reward_support_min = 0; e.cfg.reward_support_max = Sr - 1;
  e.cfg.no_target_transform = 0;
  e.A = A; e.O = O; e.split_f16 = split != 0;
  e.shape = nullptr;
  for (const SearchShape &r : g_rows) if (A <= r.amax) { e.shape = &r; break; }
  if (!e.shape) return fail("no row for %d actions", A);
  e.jtp = e.shape->jtp;
  e.pack_idx_h2 = nullptr; e.n_packed_h2 = 0;
  return build_packing(&e);
}
static void release(mz_engine &e) { for (void *p : e.allocs) free(p); e.allocs.clear(); }
int main(int argc, char **argv) {
  mz_engine e;
  if (argc == 3 && !strcmp(argv[1], "--time")) {
    const int n = atoi(argv[2]);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) { if (build(e, 8, 4, 31, 31, 0)) return 1; release(e); }
    printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n);
    return 0;
  }
  int O, A, Sv, Sr, split;
  while (scanf("%d %d %d %d %d", &O, &A, &Sv, &Sr, &split) == 5) {
    if (build(e, O, A, Sv, Sr, split)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    const float *P = e.packed;
    const NetView &n = e.nv;
    const long long rec[MZ_FIELDS] = {
        (long long)e.n_flat, (long long)e.n_packed, (const float *)n.w0o - P, n.b0o - P, (const float *)n.w1 - P, (const float *)n.b1 - P,
        (const float *)n.w2 - P, n.b2 - P, (const float *)n.w3 - P, (const float *)n.b3 - P, (const float *)n.w4 - P, n.b4 - P, n.lnw - P,
        n.lnb - P, (long long)g_locals[0], (long long)g_locals[1], (const float *)e.wstream - P, (long long)g_locals[2],
        (long long)g_locals[3], (const float *)e.istream - P, (long long)g_locals[4], (long long)e.n_packed_h2, n.ks0, n.ks1, n.ks3,
        (long long)g_locals[5], e.nst0, (long long)g_locals[6], (long long)(e.n_packed_h2 / (4 * 8 * 512))};
    fwrite(rec, sizeof rec, 1, stdout);
    fwrite(e.pack_idx, 4, e.n_packed, stdout);
    fwrite(e.pack_idx2, 4, e.n_packed, stdout);
    if (e.n_packed_h2) fwrite(e.pack_idx_h2, 4, e.n_packed_h2, stdout);
    release(e);
  }
  return 0;
}
'''


def parent_program(tmp):
  show = lambda path: subprocess.check_output(['git', 'show', '%s:%s' % (PARENT, path)], cwd=ROOT, text=True)
  lines = show(ENGINE).split('\n')
  part = ['\n'.join(lines[a - 1:b]) + '\n' for a, b in RANGES]
  hook = '  e->n_packed = pos;\n'
  assert part[2].count(hook) == 1
  part[2] = part[2].replace(hook, hook + '  { const size_t l_[7] = {p_w1f, p_w3f, p_h4, p_p4, wstride, (size_t)nsteps, (size_t)nroot}; memcpy(g_locals, l_, sizeof l_); }\n')
  kernels = show('model-based-rl_amd/csrc/mz_kernels.inc')
  src = os.path.join(tmp, 'pack_parent.cpp')
  with open(src, 'w') as f:
    f.write('#define MZ_FIELDS %d\n' % FIELDS + STUBS.replace('struct FlatLayout;\n', part[0]) + kernels + ENGINE_STUB + part[1] + part[2] + MAIN)
  exe = os.path.join(tmp, 'pack_parent')
  subprocess.check_call(['g++', '-std=c++17', '-O2', src, '-o', exe])
  return exe


def digests(blob, all_cases):
  """per case the four digests, from the program's output: record, idx, idx2, idx_h2 back to back"""
  out, at = {}, 0
  for case in all_cases:
    rec = blob[at:at + 8 * FIELDS]
    at += 8 * FIELDS
    fields = struct.unpack('<%dq' % FIELDS, rec)
    n, nh = fields[1], fields[21]
    tabs = []
    for size in (n, n, nh):
      tabs.append(hashlib.sha256(blob[at:at + 4 * size]).hexdigest() if size else None)
      at += 4 * size
    out[key(case)] = {'record': hashlib.sha256(rec).hexdigest(), 'idx': tabs[0], 'idx2': tabs[1], 'idx_h2': tabs[2]}
  assert at == len(blob), (at, len(blob))
  return out


def main():
  with tempfile.TemporaryDirectory() as tmp:
    exe = parent_program(tmp)
    if len(sys.argv) == 3 and sys.argv[1] == '--time':
      print(subprocess.check_output([exe, '--time', sys.argv[2]], text=True).strip())
      return
    all_cases = cases()
    found = {}
    for at in range(0, len(all_cases), 20):      # (a case's tables are ~7 MB)
      chunk = all_cases[at:at + 20]
      blob = subprocess.run([exe], input=''.join('%d %d %d %d %d\n' % c for c in chunk).encode(), stdout=subprocess.PIPE, check=True).stdout
      found.update(digests(blob, chunk))
  golden = {'parent': PARENT, 'cases': found}
  path = os.path.join(ROOT, 'tests', 'golden', 'pack_sha256.json')
  with open(path, 'w') as f:
    json.dump(golden, f, indent=0, sort_keys=True)
    f.write('\n')
  print('%d cases -> %s' % (len(all_cases), path))


if __name__ == '__main__':
  main()
