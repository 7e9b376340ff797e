#!/usr/bin/env python3
"""Headline benchmark: self-play env-steps/sec at num_simulations=30 (BASELINE.json).

One "step" = one complete move of every environment on this rank: observation -> initial inference ->
root expand + Dirichlet noise -> 30 x {select, recurrent inference, expand, backup} -> action sampling ->
env.step -> experience record; records are drained D2H into pinned memory and ingested by the host
prioritized replay (the reference's own metric: experiences accepted by save_history per wall-second,
replay_buffer.py:121 / learners.py:94-109).  N > 1: one process per GPU, environments sharded by global env
id, weights broadcast from rank 0 over RCCL; no data-path collective (scaling = weak).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      bench.py --gpus N --steps K --warmup W
Prints ONE JSON line on rank 0.

A plain run sets up, primes and warms up, times ONE region of exactly K steps and prints the headline.  --full adds what
takes runs of its own: 5 timed regions of >= 1.2 s each (mean +- std), the search kernel's roofline (HIP-event clock and,
N = 1, the rocprofv3 traffic passes), the split-f16 and policy-gain depth secondaries, the one-replay layout of N > 1 and
the CPU baselines.  --dump-outputs DIR: rank 0's experience records of the last timed step, one DIR/<field>.npy per field.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

# BASELINE.json configs[1] (the headline, default): LunarLander-v2 shapes, FCNetwork, 30 simulations, 4096 parallel
# envs per GPU.  Secondary lines for profiles/, never the headline: --workload pong = configs[3]'s shapes on one GPU
# (Pong-ram: 128 uint8 observations with --norm_obs 0 255, 6 actions, 50 simulations); --workload breakout =
# configs[4] (MuZeroNetwork through PyTorch-ROCm behind the external-inference entry points, bench_torch.py);
# --workload tree = the stand-alone tree kernels of that path against the HBM / cache rooflines (bench_tree.py);
# --workload learner = the learner step (row f2) in Learner.learn's loop (bench_learner.py).
WORKLOADS = {'lunar': ('LunarLander-v2', 4096, 8, 4, 30, 256), 'pong': ('Pong-ramNoFrameskip-v4', 4096, 128, 6, 50, 1024),
             # configs[0]'s game at throughput size (SURVEY.md s8d Config 1): TicTacToe with the reference's rules ON THE DEVICE,
             # two players, known bounds (-1, 1), discount 1; games last 5-9 moves
             'tictactoe': ('TicTacToe', 4096, 9, 9, 30, 9)}
WNAME, B, O, A, SIMS, EPISODE_LEN = WORKLOADS['lunar']
for _i, _a in enumerate(sys.argv):
  if _a == '--workload' and _i + 1 < len(sys.argv) and sys.argv[_i + 1] in WORKLOADS:
    WNAME, B, O, A, SIMS, EPISODE_LEN = WORKLOADS[sys.argv[_i + 1]]
  if _a == '--envs' and _i + 1 < len(sys.argv):
    B = int(sys.argv[_i + 1])                # (tests: a small pool; the line then says so in config.envs_per_gpu)
CHUNK = 16                      # moves per drain/ingest chunk = whole moves per launch of the search kernel (8 until r03_i: +0.5 %)
FLOP_PER_SIM = 2 * 512 * (312 + 3 * A)            # 331 776 for A = 4
FLOP_PER_ROOT = 2 * 512 * (O + 181 + A)           # 197 632 for O = 8, A = 4
PEAK_F32_MFMA_TFLOPS = 157.3                      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense


def _usable_cores():
  """cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes expose
  256 logical CPUs but run the job under a 16-CPU quota; threads beyond the quota only time-slice)."""
  n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
  try:
    quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
    if quota != 'max':
      n = min(n, max(1, int(int(quota) / int(period))))
  except (OSError, ValueError):
    pass
  return n


def cpu_baseline(weights):
  """The CPU oracle (C restatement of the reference path, oracle/mz_oracle.c) timed on the host cores on a bounded
  sample of the same workload: one thread per usable core (up to 64), every thread its own batch of environments -- the
  layout of the reference's Ray actors (one single-threaded process per actor, train.py:63,72).  The C call releases
  the GIL.  Reported beside the GPU number; it is not the target."""
  import threading
  from oracle import oracle as orc
  envs, moves = 256, 24       # ~10 s of work per core
  cores = max(1, min(64, _usable_cores()))
  net = orc.FCNet(weights, O, A)

  def make(seed):
    rng = np.random.RandomState(seed)
    t = orc.Trees(orc.tree_cfg(A, SIMS), envs)
    obs = rng.standard_normal((envs, O)).astype(np.float32)
    noise = rng.dirichlet([0.25] * A, size=envs)
    return rng, t, obs, noise

  def work(state, n):
    rng, t, obs, noise = state
    for _ in range(n):
      t.search_fc(net, obs, np.ones(envs, np.int8), None, noise, 0.25)
      t.finalize(1.0, rng.uniform(size=envs))

  one = make(0)
  work(one, 1)                # warm-up
  t0 = time.perf_counter()
  work(one, moves // 4)
  dt1 = time.perf_counter() - t0
  single = envs * (moves // 4) / dt1
  states = [make(i) for i in range(cores)]
  for st in states:
    work(st, 1)
  threads = [threading.Thread(target=work, args=(st, moves)) for st in states]
  t0 = time.perf_counter()
  for th in threads:
    th.start()
  for th in threads:
    th.join()
  dt = time.perf_counter() - t0
  return {'value': cores * envs * moves / dt, 'unit': 'env-steps/s', 'cores': cores, 'kind': 'port',
          'sample': '%d threads x %d envs x %d moves x %d simulations, oracle/mz_oracle.c (gcc -O2, scalar float32 net + '
                    'double tree), %.1f s' % (cores, envs, moves, SIMS, dt),
          'single_core_value': single, 'host_cpus': os.cpu_count(), 'usable_cores': _usable_cores(),
          'cpu_model': _cpu_model()}


def _cpu_model():
  try:
    for line in open('/proc/cpuinfo'):
      if line.startswith('model name'):
        return line.split(':', 1)[1].strip()
  except OSError:
    pass
  return 'unknown'


def cpu_baseline_reference_shaped():
  """The reference's own shape of the path on the host cores: oracle/ref_shaped.py (batch-1 PyTorch-CPU restatement
  of actors.py:131-153 + mcts.py:78-143, one environment per single-threaded process -- the reference's Ray actor
  layout, train.py:63,72), one process per usable core.  Its fidelity to the imported reference is measured in the
  build container (scripts/ref_shaped_ratio.py -> profiles/r02_ref_shaped_ratio.json: ratio 1.02-1.04).  The children
  are fresh interpreters that never touch the GPU."""
  import subprocess
  cores = max(1, min(64, _usable_cores()))
  moves = 600 if SIMS <= 30 else 350          # ~8-10 s per process
  env = dict(os.environ, OMP_NUM_THREADS='1', MKL_NUM_THREADS='1', HIP_VISIBLE_DEVICES='', ROCR_VISIBLE_DEVICES='')
  cmd = [sys.executable, os.path.join(ROOT, 'oracle', 'ref_shaped.py'), '--obs', str(O), '--actions', str(A), '--sims',
         str(SIMS), '--moves', str(moves)]
  t0 = time.perf_counter()
  procs = [subprocess.Popen(cmd + ['--seed', str(i)], stdout=subprocess.PIPE, env=env) for i in range(cores)]
  rates = []
  for pr in procs:
    out = pr.communicate(timeout=600)[0].decode().strip().splitlines()
    if pr.returncode == 0 and out:
      rates.append(json.loads(out[-1])['env_steps_per_s'])
  wall = time.perf_counter() - t0
  if not rates:
    return None
  return {'value': float(np.sum(rates)), 'unit': 'env-steps/s', 'cores': len(rates), 'kind': 'reference-shaped',
          'per_core_value': float(np.mean(rates)),
          'sample': '%d single-threaded processes x 1 env x %d moves x %d simulations, oracle/ref_shaped.py (batch-1 '
                    'PyTorch-CPU, the reference\'s op sequence), %.1f s wall incl. interpreter start' % (len(rates), moves, SIMS, wall),
          'fidelity': 'profiles/r02_ref_shaped_ratio.json (timed beside the imported reference in the build container)'}


def build_id():
  """what this line was measured ON: a hash over the kernel / host sources and this file (the GPU box has no .git: a commit id is
  not available there).  An N > 1 line looks for an N = 1 line of the same build under profiles/ (efficiency_vs_n1)."""
  import glob
  import hashlib
  h = hashlib.sha256()
  pkg = os.path.join(ROOT, 'model-based-rl_amd')
  files = sorted(glob.glob(os.path.join(pkg, 'csrc', '*.hip')) + glob.glob(os.path.join(pkg, 'csrc', '*.h')) +
                 glob.glob(os.path.join(pkg, 'csrc', '*.inc')) + glob.glob(os.path.join(pkg, 'csrc', '*.cpp')) +
                 glob.glob(os.path.join(pkg, '*.py')) + [os.path.abspath(__file__)])
  for f in files:
    h.update(os.path.basename(f).encode())
    h.update(open(f, 'rb').read())
  return h.hexdigest()[:16]


def n1_reference(workload, one_replay):
  """the N = 1 line of this workload under profiles/ (files named *_bench*.json): the one of the same build if there is one, else the
  newest; -> (value, same_build, file) or None"""
  import glob
  bid, best = build_id(), None
  for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*bench*.json')), key=os.path.getmtime):
    try:
      line = json.load(open(f))
    except (ValueError, OSError):
      continue
    if not isinstance(line, dict) or line.get('n_gpus') != 1 or line.get('unit') != 'env-steps/s' or line.get('secondary') or line.get('secondary_line'):
      continue
    if not str(line.get('config', {}).get('workload', '')).startswith(workload) or line.get('config', {}).get('envs_per_gpu') != B:
      continue
    same = line.get('build_id') == bid
    if best is None or same or not best[1]:
      best = (float(line['value']), same, os.path.basename(f))
  return best


def efficiency_vs_n1(value, world, one_replay):
  """value / (N x the N = 1 line's value) where profiles/ holds one (the driver computes its own from its per-N runs; this is
  for reading a lone N > 1 record)"""
  if world <= 1:
    return None
  ref = n1_reference(WNAME, one_replay)
  if ref is None:
    return None
  return {'efficiency': value / (world * ref[0]), 'n1_value': ref[0], 'n1_file': ref[2], 'same_build': ref[1]}


def preflight_or_exit(world):
  """before ANY GPU call of a multi-rank run: devices, shared memory for the experience rings of the
  one-replay layout, host cores -- distributed.preflight; one sentence and a non-zero exit otherwise"""
  from model_based_rl_amd import distributed as D
  ram = '-ram' in WNAME
  rec = ((O + 3) // 4 if ram else O) + A + 10
  shared = os.environ.get('MZ_BENCH_BACKEND', 'nccl') == 'gloo' or os.environ.get('MZ_SHARED_GPU_OK', '0')[:1] == '1'
  need = int(os.environ.get('MZ_PREFLIGHT_SHM_NEED', '0')) or D.ring_bytes(world, CHUNK, B, rec)      # (MZ_PREFLIGHT_SHM_NEED: tests)
  return D.preflight(world, shm_need=need, ingest_threads=ingest_threads_for(world, one_replay_rank0=True) if world > 1 else 0,
                     shared_gpu_ok=shared)


def bench_config(workload_name, envs, sims, episode_len, world, sync_every, ingest_threads, split_f16=False, run_tag='bench'):
  """The run's Config, from the flags `python -m model_based_rl_amd.train` takes (reference config.py:87-231 names): what
  Actor / PrioritizedReplay / SharedStorage are constructed from below, exactly as train.launch constructs them."""
  import tempfile
  from model_based_rl_amd.config import make_config
  argv = ['--environment', workload_name, '--num_envs', str(envs), '--num_simulations', str(sims), '--episode_length', str(episode_len),
          '--seed', '1234', '--num_actors', str(world), '--window_size', str(1 << 21), '--batch_size', '256', '--num_unroll_steps', '5',
          '--td_steps', '10', '--max_history_length', '500', '--weight_sync_frequency', str(sync_every), '--ingest_threads', str(ingest_threads),
          '--runs_dir', os.path.join(tempfile.gettempdir(), 'mz_bench_runs'), '--run_tag', run_tag, '--actor_log_frequency', '1',
          '--fixed_temperatures'] + ['1.0'] * world      # (T = 1 whatever training step the weight publisher has reached)
  if workload_name == 'TicTacToe':
    argv += ['--two_players', '--known_bounds', '-1', '1', '--discount', '1']
  if '-ram' in workload_name:          # the -ram- envs: byte observations, --norm_obs --obs_range 0 255 (actors.py:55-58,134-137)
    argv += ['--norm_obs', '--obs_range', '0', '255']
  if split_f16:
    argv += ['--split_f16']
  return make_config(argv)


class WeightPublisher(object):
  """Stand-in for the learner where none runs ("weight broadcast ... timer-driven if no learner"): a thread on
  the storage rank that does what Learner.send_weights does (learners.py:85-86,132-133) -- storage.store_weights(weights,
  training_step) with a growing step -- every `period` seconds, so that the actors' pulls (Actor.sync_weights, actors.py:81-85)
  find a new training step and really reload + repack inside the timed regions."""

  def __init__(self, storage, weights, period=0.1):
    import threading
    from model_based_rl_amd.actors import _call
    self.storage, self.weights, self.period, self.step, self._call = storage, weights, period, 0, _call
    self.stop = threading.Event()
    self.publish()
    self.thread = threading.Thread(target=self._run, daemon=True)
    self.thread.start()

  def publish(self):
    self.step += 1
    self._call(self.storage, 'store_weights', self.weights, self.step)

  def _run(self):
    while not self.stop.wait(self.period):
      self.publish()

  def close(self):
    self.stop.set()
    self.thread.join(timeout=5)


def _under_profiler():
  pre = os.environ.get('LD_PRELOAD', '')
  return any(k.startswith(('ROCPROF', 'ROCP_', 'ROCTRACER')) for k in os.environ) or 'rocprof' in pre


def live_traffic(workload, split_f16, chunk):
  """HBM-side bytes per launch of the search kernel, measured in THIS run: two child processes -- `rocprofv3 --pmc FETCH_SIZE`
  and `--pmc WRITE_SIZE` (separate passes, counters only, the program itself behind `--`) around a short run of this very
  script -- started BEFORE this process touches the GPU.  bytes = 1024 * (2 * FETCH_SIZE + WRITE_SIZE) per launch (KB units
  and the gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md, as scripts/make_traffic.py does).  None where rocprofv3 is
  missing, the passes fail, or this process is itself being profiled."""
  import csv, glob, shutil, subprocess, tempfile
  if _under_profiler() or os.environ.get('MZ_BENCH_CHILD') or not shutil.which('rocprofv3'):
    return None
  kernel = 'k_search_h2' if split_f16 else 'k_search_fused'
  means = {}
  for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
    d = tempfile.mkdtemp(prefix='mz_pmc_', dir='/tmp')
    cmd = ['rocprofv3', '--pmc', counter, '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--steps', str(chunk), '--warmup', str(chunk), '--no-cpu-baseline', '--min-seconds', '0.05', '--workload', workload, '--full',
           '--chunk', str(chunk)] + (['--split-f16'] if split_f16 else [])
    try:
      subprocess.run(cmd, env=dict(os.environ, MZ_BENCH_CHILD='1', TMPDIR='/tmp'), cwd='/tmp', stdout=subprocess.DEVNULL,
                     stderr=subprocess.DEVNULL, timeout=90)
      n, tot = 0, 0.0
      for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
        for row in csv.DictReader(open(f, newline='')):
          if row.get('Counter_Name') == counter and row.get('Kernel_Name', '').replace('void ', '').startswith(kernel):
            n += 1
            tot += float(row['Counter_Value'])
      if n:
        means[counter] = (tot / n, n)
    except Exception:
      pass
    finally:
      shutil.rmtree(d, ignore_errors=True)
  if len(means) != 2:
    return None
  return {'bytes_per_launch': 1024.0 * (2.0 * means['FETCH_SIZE'][0] + means['WRITE_SIZE'][0]),
          'launches': [means['FETCH_SIZE'][1], means['WRITE_SIZE'][1]]}


def measure_actor(device, weights, chunk, moves=384, split_f16=False, run_tag='bench_secondary'):
  """Short measurement of the headline workload with another weight set / kernel variant, through the SAME product loop as `value`
  -- an Actor of its own (storage, native replay) driven by Actor.launch: frames accepted by the replay per second over `moves`
  moves, and the search kernel's launch duration (HIP events on its dispatches)."""
  from model_based_rl_amd import rayshim as ray
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = bench_config(WNAME, B, SIMS, EPISODE_LEN, 1, 1 << 20, ingest_threads_for(1), split_f16=split_f16, run_tag=run_tag)
  cfg.selfplay_chunk = chunk
  storage, replay = ray.remote(SharedStorage).remote(cfg), ray.remote(PrioritizedReplay).remote(cfg)
  storage.store_weights.remote(weights, 1).result()
  actor = Actor(0, cfg, storage, replay)
  eng = actor.engine
  moves = (moves // chunk) * chunk
  # priming (every env past its first, partial episode; the replay's window filled once, as for `value`) + warm-up
  actor.launch(max(EPISODE_LEN, min(int(cfg.window_size) // B + chunk, 1024)) + 64)
  torch.cuda.synchronize(device)
  f0 = replay.get_throughput.remote().result()['frames']
  t0 = time.perf_counter()
  actor.launch(moves)
  torch.cuda.synchronize(device)
  dt = time.perf_counter() - t0
  frames = replay.get_throughput.remote().result()['frames'] - f0
  pinned = actor._pipe.pinned[0]
  durs = []
  for _ in range(3):
    durs += eng.selfplay_steps_timed(chunk)
    eng.selfplay_drain(pinned, chunk)
    torch.cuda.synchronize(device)
  us = 1e3 * float(np.mean(durs[chunk:]))
  persistent = eng.selfplay_moves_per_launch() > 0      # whole moves inside the launch: `us` then includes the (f32) root
  actor.close()
  eng.close()
  return {'env_steps_per_s': frames / dt, 'counted': 'frames accepted by the replay (Actor.launch, the same loop as `value`)',
          'env_steps_executed_per_s': B * moves / dt, 'ms_per_step': 1e3 * dt / moves,
          'kernel_us_per_move': us, 'root_inside_the_launch': persistent, 'moves': moves,
          'algorithmic_tflops': (SIMS * FLOP_PER_SIM + (FLOP_PER_ROOT if persistent else 0)) * B / (us * 1e-6) / 1e12}


def measure_split_f16(device, weights, chunk, moves=384):
  """the opt-in split-f16 search kernel (mz_config.split_f16, `--split_f16`) on the headline workload (measure_actor)"""
  out = {'what': 'mz_config.split_f16 = 1: FCNetwork GEMMs as float16 high/low splits on v_mfma_f32_16x16x32_f16, f32 '
                 'accumulation; float32-level accuracy (every parity test passes), not bit-identical to the exact-f32 path'}
  out.update(measure_actor(device, weights, chunk, moves, split_f16=True, run_tag='bench_split_f16'))
  return out


def sharpened(weights, gain):
  """the weight set with the policy head's output layer times `gain`: logits x gain => sharper priors => the search commits to
  fewer children and descends deeper -- what a TRAINED policy does to the tree (the reference's actors run trained weights,
  actors.py:81-85; the headline runs torch.manual_seed(0) weights as SURVEY.md s8d prescribes).  Parity is untouched: it is a
  weight set like any other."""
  w = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in weights.items()}
  for k in ('policy_head.policy.weight', 'policy_head.policy.bias'):
    w[k] = w[k] * float(gain)
  return w


def leaf_depths(eng, obs_dim, n_trees):
  """mean / max depth of the leaves one search expands (one move of `n_trees` trees of this engine): node n > 0 is child
  (n - 1) % A of the node with expansion index (n - 1) // A; expansion indices are assigned in order"""
  eng.initial_inference(torch.randn(n_trees, obs_dim, device=eng.device))
  eng.root_prepare(None, None, None, device_rng=True, move=0)
  eng.search()
  E = eng.export_tree()['E']
  A_ = eng.A
  ds = []
  for b in range(E.shape[0]):
    nodes = np.flatnonzero(E[b] >= 0)
    dep = {0: 0}
    for e, n in sorted((int(E[b, n]), int(n)) for n in nodes if n != 0):
      dep[e] = dep[(n - 1) // A_] + 1
    ds += [v for k, v in dep.items() if k != 0]
  ds = np.array(ds)
  return float(ds.mean()), int(ds.max())


def depth_sensitivity(device, weights, chunk, gains=(1, 4, 24, 96)):
  """the headline at realistic tree depth.  For every policy gain: env-steps/s through Actor.launch, the search
  kernel's roofline fraction, mean / max leaf depth of a search, and the two phases of a simulation that grow with depth -- the
  descent (`t_select`) and the barrier wait for the deepest of a workgroup's 16 trees (`bar`) -- from the stamped build
  (mz_search_phase_profile: cycles per simulation, wave 0, mean over workgroups).  Gains 24 and 96 put the mean leaf depth at ~4 and
  ~6 (scripts/experiments/policy_gain_depth_probe.py: 1 -> 2.5, 8 -> 3.0, 24 -> 4.1, 48 -> 5.1, 128 -> 6.4), the Pong-ram / TicTacToe
  shapes' depths with random-init weights are 3.7 / 5.3."""
  from model_based_rl_amd.engine import Engine
  rows = []
  base = None
  for g in gains:
    w = sharpened(weights, g)
    m = measure_actor(device, w, chunk, moves=256, run_tag='bench_gain_%g' % g)
    eng = Engine(B, O, A, SIMS, seed=1, device=device)
    eng.set_weights(w)
    mean_d, max_d = leaf_depths(eng, O, B)
    obs = torch.randn(B, O, device=device)
    for it in range(2):
      eng.initial_inference(obs); eng.root_prepare(None, None, None, device_rng=True, move=it)
      c = eng.search_phase_profile()
    eng.close()
    cyc = {'bar': float(c[0, 1]) / SIMS, 't_select': float(c[0, 12]) / SIMS, 't_backup': float(c[0, 11]) / SIMS, 'total': float(c[0].sum()) / SIMS}
    row = {'policy_gain': g, 'env_steps_per_s': m['env_steps_per_s'], 'kernel_us_per_move': m['kernel_us_per_move'],
           'frac': m['algorithmic_tflops'] / PEAK_F32_MFMA_TFLOPS, 'mean_leaf_depth': mean_d, 'max_leaf_depth': max_d, 'cycles_per_sim_wave0': cyc}
    if base is None:
      base = row
    else:
      added = cyc['total'] - base['cycles_per_sim_wave0']['total']
      row['added_cycles_per_sim'] = added
      row['share_of_added'] = {k: (cyc[k] - base['cycles_per_sim_wave0'][k]) / added if added > 0 else None for k in ('bar', 't_select', 't_backup')}
    rows.append(row)
  return {'what': 'policy-head output layer x gain (sharper priors => deeper trees; random-init weights otherwise): the LunarLander-shape '
                  'line at the tree depths a trained policy produces; gain 1 = the headline\'s weights',
          'rows': rows}


def ingest_threads_for(world, one_replay_rank0=False):
  """Ingest threads of a rank's native replay, sized so that `world` ranks fit the box's usable cores (the GPU boxes run a job
  under a 16-CPU quota): every rank keeps its launching thread and its ingest worker (~1.2 cores busy); what is
  left of the rank's share -- at most 4 -- assembles histories.  One thread sustains 42-46 M records/s against the 10 M/s a
  GPU produces (profiles/r03_*_ingest_bench.json).  one_replay_rank0: the ONE replay of `--one-replay` takes every other
  rank's records too and gets the cores the other ranks leave."""
  cores = _usable_cores()
  if one_replay_rank0:
    return int(max(1, min(8, cores - 1.25 * world)))
  return int(max(1, min(4, cores // max(1, world) - 1)))


def dump_outputs(dirname, rec, obs_u8):
  """--dump-outputs: one move of experience records [B, rec_floats] -- what Actor.launch hands the replay for the last timed
  step -- as one DIR/<field>.npy per field of engine.records_view: the float fields as they are (float32, root value and
  error float64), the integer fields as float64 (exact)"""
  from model_based_rl_amd.engine import records_view
  os.makedirs(dirname, exist_ok=True)
  for name, v in records_view(rec, O, A, obs_u8=obs_u8).items():
    v = np.asarray(v)
    if v.dtype not in (np.float32, np.float64):
      v = v.astype(np.float64)
    np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(v))


def self_launch(args):
  """`python bench.py --gpus N` with N > 1 and no launcher: start `python -m torch.distributed.run --nproc-per-node N bench.py
  ...` as a CHILD process (this process has not touched the GPU -- and never replaces itself: os.exec* from a GPU process takes
  the box down), relay rank 0's JSON line and exit with the child's code.  (Reference wiring: train.py:62-78 starts N actor
  processes from one command.)"""
  import socket
  import subprocess
  with socket.socket() as sk:
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus), '--master-addr',
         '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
  env = dict(os.environ)
  env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  env.setdefault('OMP_NUM_THREADS', '1')
  proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
  line = None
  for out in proc.stdout:
    out = out.rstrip('\n')
    if out.startswith('{') and '"metric"' in out:
      line = out
    else:
      print(out, file=sys.stderr, flush=True)
  rc = proc.wait()
  if line is not None:
    print(line, flush=True)
  sys.exit(rc if rc else (0 if line is not None else 1))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  ap.add_argument('--steps', type=int, default=512)
  ap.add_argument('--warmup', type=int, default=64)
  ap.add_argument('--no-cpu-baseline', action='store_true')
  ap.add_argument('--workload', choices=sorted(WORKLOADS) + ['breakout', 'tree', 'learner'], default='lunar')
  ap.add_argument('--envs', type=int, default=None, help='override the number of environments per GPU (tests)')
  ap.add_argument('--chunk', type=int, default=CHUNK, help='moves per drain / ingest chunk')
  ap.add_argument('--sync-every', type=int, default=128,
                  help='moves between weight pulls (the path\'s one exchange: broadcast + repack)')
  ap.add_argument('--publish-period', type=float, default=0.02,
                  help='seconds between the weight publisher\'s store_weights calls on rank 0 (stand-in for Learner.send_weights)')
  ap.add_argument('--min-seconds', type=float, default=None,
                  help='the --steps block is repeated back to back until one timed region is at least this long '
                       '(default: 0 -- the region is exactly --steps steps; 1.2 with --full)')
  ap.add_argument('--runs', type=int, default=None,
                  help='timed regions; `value` covers all of them (default: 1; 5 with --full -- SURVEY.md s8d: mean +- std of 5 runs)')
  ap.add_argument('--full', action='store_true',
                  help='everything beyond the headline: 5 regions of >= 1.2 s, roofline (kernel clock, live traffic), the split-f16 '
                       'and depth secondaries, the one-replay layout of N > 1, the CPU baselines')
  ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                  help='write rank 0\'s experience records of the last timed step as DIR/<field>.npy (float32 / float64)')
  ap.add_argument('--split-f16', action='store_true',
                  help='secondary line: the FCNetwork GEMMs as float16 high/low splits on the f16 matrix pipe '
                       '(mz_config.split_f16; float32-level accuracy, not bit-identical to the exact-f32 default)')
  ap.add_argument('--one-replay', action='store_true',
                  help='N > 1: `value` in the topology of `train --ranks N` -- every rank ships its record chunks through a '
                       'shared-memory ring to rank 0, whose ONE native replay ingests them all (default: one replay per rank, '
                       'and this layout as `one_replay_secondary` in the same line; DESIGN.md s6)')
  ap.add_argument('--no-one-replay-secondary', action='store_true')
  ap.add_argument('--ingest-threads', type=int, default=None, help='ingest threads per replay (default: from usable cores / ranks)')
  ap.add_argument('--no-live-traffic', action='store_true',
                  help='do not measure roofline.traffic with two rocprofv3 --pmc child runs (N = 1 only; ~20 s)')
  ap.add_argument('--policy-gain', '--policy_gain', type=float, default=1.0,
                  help='policy-head output layer x gain for the WHOLE run (sharper priors, deeper trees; secondary line when != 1)')
  ap.add_argument('--no-depth-sensitivity', action='store_true',
                  help='skip the depth_sensitivity block (N = 1, default workload: four short runs at policy gains 1, 4, 24, 96; ~10 s)')
  ap.add_argument('--batch', default=None,
                  help='--workload learner: batch sizes of the sweep, comma separated (default 256,512,1024,2048,4096; the line\'s `value` '
                       'stays the first one -- 256 = the reference\'s batch_size): updates/s, samples/s, roofline.frac and host us per update each')
  ap.add_argument('--dump-records', default=None,
                  help='(tests) save this rank\'s experience records of the first moves after reset to <path>.rank<r>.npy')
  args = ap.parse_args()
  selfplay = args.workload in WORKLOADS          # (the other workloads are lines of their own, unchanged by --full)
  if args.runs is None:
    args.runs = 5 if args.full or not selfplay else 1
  if args.min_seconds is None:
    args.min_seconds = 1.2 if args.full or not selfplay else 0.0
  if args.dump_outputs and not selfplay:
    ap.error('--dump-outputs covers the self-play workloads (%s)' % ', '.join(sorted(WORKLOADS)))
  if args.workload == 'breakout':
    import bench_torch             # secondary line: MuZeroNetwork through PyTorch-ROCm (BASELINE.json configs[4])
    return bench_torch.main(args)
  if args.workload == 'tree':
    import bench_tree              # secondary line: the stand-alone tree kernels against the HBM / cache rooflines (SURVEY.md s8d ii)
    return bench_tree.main(args)
  if args.workload == 'learner':
    import bench_learner           # secondary line: the learner step in Learner.learn's loop
    return bench_learner.main(args)
  if args.gpus > 1 and 'RANK' not in os.environ:
    preflight_or_exit(args.gpus)   # (before the ranks exist: one sentence instead of N tracebacks)
    return self_launch(args)       # one process per GPU, started from here (before anything touches the GPU)
  chunk = max(1, args.chunk)
  child = bool(os.environ.get('MZ_BENCH_CHILD'))     # a PMC pass of live_traffic(): every launch must play `chunk` moves

  world = int(os.environ.get('WORLD_SIZE', '1'))
  rank = int(os.environ.get('RANK', '0'))
  preflight = preflight_or_exit(world) if world > 1 else None      # every rank, before it touches its GPU (launcher-started runs)
  # roofline.traffic, live: the two PMC passes run as child processes before this process initialises the GPU
  measured_traffic = None
  if args.full and world == 1 and 'RANK' not in os.environ and not args.no_live_traffic and not args.envs:
    measured_traffic = live_traffic(args.workload, args.split_f16, chunk)
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  dist = None
  backend = None
  # MZ_BENCH_FORCE_DIST=1: take the multi-rank branch at ANY world size (launched by torch.distributed.run with one
  # process it runs the whole collective path -- process group over RCCL, broadcast of the weights into device memory,
  # the MAX / SUM all-reduces, barriers -- on a single GPU)
  force_dist = os.environ.get('MZ_BENCH_FORCE_DIST', '0')[:1] == '1' and 'RANK' in os.environ
  # stdout carries the ONE JSON line: everything else this process prints there -- the product's "Actor-k is online ...", RCCL's
  # version banner, gloo's connection notes (C-level writes to descriptor 1) -- goes to stderr until the line is due
  sys.stdout.flush()
  saved_stdout = os.dup(1)
  os.dup2(2, 1)
  if world > 1 or force_dist:
    import torch.distributed as dist
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    local_rank = local_rank % max(1, torch.cuda.device_count())   # (several ranks on one GPU only in the gloo self-test)
    torch.cuda.set_device(local_rank)
    backend = os.environ.get('MZ_BENCH_BACKEND', 'nccl')             # 'nccl' = RCCL over xGMI; 'gloo' for the 1-GPU self-test
    if backend == 'nccl':
      # (no device_id: the group's own RCCL communicator is created lazily, i.e. never -- the weights travel on the library's
      # communicator, distributed.RankStorage, everything else over its host-side group; MZ_TORCH_COLLECTIVES=1 uses this one)
      dist.init_process_group('nccl')
    else:
      dist.init_process_group(backend)
  device = torch.device('cuda', local_rank)
  torch.cuda.set_device(device)
  coll_dev = device if backend != 'gloo' else torch.device('cpu')     # where collective buffers live

  import contextlib
  from model_based_rl_amd import rayshim as ray
  from model_based_rl_amd import distributed as D
  from model_based_rl_amd.actors import Actor, _call
  from model_based_rl_amd.engine import flatten_weights
  from model_based_rl_amd.networks import FCNetwork
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  from model_based_rl_amd.distributed import rccl_mapped

  # ---- the product's own objects, wired as train.launch / train.launch_ranks wire them (reference train.py:62-78): a
  # SharedStorage and a PrioritizedReplay behind actor handles, one Actor per rank (one GPU each); everything below only calls
  # Actor.launch(moves) -- the launch-ahead record pipeline, the game statistics, the ingest and the weight pulls
  # (Actor.sync_weights every --sync-every moves) are the Actor's (model-based-rl_amd/actors.py)
  game = WNAME == 'TicTacToe'
  ram = '-ram' in WNAME
  sync_every = max(chunk, args.sync_every)
  cfg = bench_config(WNAME, B, SIMS, EPISODE_LEN, world, sync_every, args.ingest_threads or ingest_threads_for(world), split_f16=args.split_f16,
                     run_tag='bench_%s_%d_rank%d' % (os.environ.get('MASTER_PORT', 'single'), os.getpid() if world == 1 else 0, rank))
  cfg.selfplay_chunk = chunk
  # random-init FCNetwork, torch.manual_seed(0) default init; rank 0 owns the weights: they reach the actors
  # through the storage (N > 1: + one broadcast of the flat float32 buffer per pull, distributed.RankStorage)
  torch.manual_seed(0)
  net = FCNetwork(O, A, torch.device('cpu'), types.SimpleNamespace()).eval()
  weights = net.get_weights()
  if args.policy_gain != 1.0:
    weights = sharpened(weights, args.policy_gain)
    net.load_state_dict(weights)
  n_flat = int(flatten_weights(weights).numel())
  storage = publisher = None
  if rank == 0:
    storage = ray.remote(SharedStorage).remote(cfg)
    # no learner in this run: its send_weights (learners.py:85-86,132-133) on a timer, often enough that every pull of the
    # actors finds a new training step and reloads + repacks
    publisher = WeightPublisher(storage, weights, period=args.publish_period)
  if dist is not None:
    from model_based_rl_amd.engine import config_scale_check
    rstorage = D.RankStorage(rank, world, device, n_flat, storage=storage, storage_call=_call, backend=backend, flatten=flatten_weights,
                             scale_check=config_scale_check(cfg))
  else:
    rstorage = storage

  # control-plane collectives (barriers, timing reductions): over the storage's host-side group where the weights travel on the
  # library's own RCCL communicator -- the process group's communicator is then never created (one proxy thread per rank)
  ctrl = getattr(rstorage, 'ctrl_group', None) if dist is not None else None
  ctrl_dev = torch.device('cpu') if ctrl is not None else coll_dev

  def barrier():
    dist.barrier(group=ctrl) if ctrl is not None else dist.barrier()

  def make_replay(threads):
    c = types.SimpleNamespace(**cfg.__dict__)
    c.ingest_threads = threads
    return ray.remote(PrioritizedReplay).remote(c)

  class Layout(object):
    """where this rank's records go: its own native replay (bench layout), or -- one_replay -- through a shared-memory
    ring to the ONE replay on rank 0 (train.launch_ranks' wiring; reference train.py:71-72: one replay buffer for all actors)"""

    def __init__(self, one_replay, tag):
      self.one_replay = one_replay
      self.rings, self.ring_stop, self.my_ring = {}, None, None
      if not one_replay:
        self.n_ingest = args.ingest_threads or ingest_threads_for(world)
        self.replay = make_replay(self.n_ingest)
        return
      import threading
      run_id = 'mzb_%s_%s' % (os.environ.get('MASTER_PORT', '0'), tag)
      self.n_ingest = args.ingest_threads or ingest_threads_for(world, one_replay_rank0=True)
      if rank == 0:
        self.rings = {r: D.ShmRing('%s_%d' % (run_id, r), chunk, B, rec_floats, slots=4, create=True) for r in range(1, world)}
      barrier()
      if rank == 0:
        self.replay = make_replay(self.n_ingest)          # (its handle serialises the two callers on rank 0: the actor and the ring server)
        self.ring_stop = threading.Event()
        threading.Thread(target=D.serve_rings, args=(self.rings, lambda name, *a: _call(self.replay, name, *a), B, self.ring_stop,
                                                     min(4, max(1, len(self.rings))), getattr(self.replay, '_obj', self.replay)),
                         daemon=True).start()
      else:
        self.my_ring = D.ShmRing('%s_%d' % (run_id, rank))
        self.replay = D.RingReplay(self.my_ring, cfg)      # (history slices assembled on this rank, as train.launch_ranks does)
        self.replay.get_throughput = lambda: {'frames': 0, 'games': 0}      # (counted where they are accepted: rank 0's replay)

    def frames(self):
      return _call(self.replay, 'get_throughput')['frames']

    def barrier(self):
      torch.cuda.synchronize(device)
      if dist is not None:
        barrier()
        if self.one_replay:   # every producer has put its last chunk: the region ends when the one replay has accepted them all
          if rank == 0:
            while any(r.pending() > 0 for r in self.rings.values()):
              time.sleep(0.0002)
            _call(self.replay, 'size')     # (queues behind an ingest in flight, and waits for the deferred insertions)
          barrier()
        torch.cuda.synchronize(device)

    def close(self):
      if self.one_replay:
        barrier()
        if self.ring_stop is not None:
          self.ring_stop.set()
        for r_ in list(self.rings.values()) + ([self.my_ring] if self.my_ring is not None else []):
          r_.release()

  def timed_regions(actor, layout, moves, n_runs):
    """n_runs timed regions, each = ONE call of Actor.launch(moves) (this rank's environments play `moves` moves; the call
    returns when the replay has taken every record), bracketed by barrier + torch.cuda.synchronize on both sides; the
    region's time is the MAX over ranks, its frames the SUM over ranks of what the replays accepted.
    -> list of (frames, seconds, host cores busy on this rank, ... max over ranks)"""
    runs = []
    for _ in range(n_runs):
      layout.barrier()
      frames0 = layout.frames()
      t0 = time.perf_counter()
      c0 = time.process_time()
      actor.launch(moves)
      layout.barrier()
      dt = time.perf_counter() - t0
      busy = (time.process_time() - c0) / dt      # CPU seconds of this rank (all its threads) per wall second
      frames = layout.frames() - frames0
      per_rank = [(float(frames), dt)]
      if dist is not None:
        mine = torch.tensor([frames, dt], dtype=torch.float64, device=ctrl_dev)
        every_r = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every_r, mine, group=ctrl)
        per_rank = [(float(x[0]), float(x[1])) for x in every_r]      # each rank's own frames and its own clock
        tt = torch.tensor([dt, busy], dtype=torch.float64, device=ctrl_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=ctrl)
        dt, busy_max = float(tt[0].item()), float(tt[1].item())
        ff = torch.tensor([frames, busy], dtype=torch.float64, device=ctrl_dev)
        dist.all_reduce(ff, op=dist.ReduceOp.SUM, group=ctrl)
        frames, busy_sum = float(ff[0].item()), float(ff[1].item())
      else:
        busy_max = busy_sum = busy
      runs.append((frames, dt, busy, busy_max, busy_sum, per_rank))
    return runs

  OS = (O + 3) // 4 if ram else O
  rec_floats = OS + A + 10                 # include/mz_engine.h: observation (packed bytes for -ram-), visit distribution, MZ_REC_EXTRA
  one_replay = bool(args.one_replay) and dist is not None and world > 1
  layout = Layout(one_replay, 'a')
  actor = Actor(rank, cfg, rstorage, layout.replay)
  eng = actor.engine
  dump = [] if args.dump_records else None
  shard = []                               # env ids of this rank's first chunk of records: [first, last]

  def tap(v):
    if not shard:
      from model_based_rl_amd.engine import records_view
      ids = records_view(v[:1], O, A, obs_u8=ram)['env_id']
      shard.extend([int(ids.min()), int(ids.max())])
    if dump is not None and len(dump) < 4:
      dump.append(v.copy())
  actor.record_tap = tap

  # priming (untimed, not part of --warmup): every env finishes its first, partial (staggered) episode, so that from here on
  # B / EPISODE_LEN episodes end per move and the replay accepts B frames per move on average -- the steady state the
  # reference's frames_per_second metric is defined on -- and the replay's window has been filled once (its storage is
  # touched: until r04 the first timed region ran 2 % below the others)
  # (a PMC child pass rounds every block to whole chunks: all its launches then play the same number of moves)
  whole = lambda n: -(-n // chunk) * chunk if child else n
  prime = max(EPISODE_LEN, min(int(cfg.window_size) // B + chunk, 1024)) if not child else EPISODE_LEN
  actor.launch(whole(prime))
  if dump is not None:
    np.save('%s.rank%d.npy' % (args.dump_records, rank), np.concatenate(dump, 0))
  actor.record_tap = dump = None
  shards = [shard]
  if dist is not None:
    st = torch.tensor(shard, dtype=torch.int64, device=ctrl_dev)
    every = [torch.zeros_like(st) for _ in range(world)]
    dist.all_gather(every, st, group=ctrl)
    shards = [[int(x[0]), int(x[1])] for x in every]
  assert eng.rec_floats == rec_floats, (eng.rec_floats, rec_floats)
  # calibration: how many --steps blocks make a timed region of >= --min-seconds (same count on every rank); none without
  # --min-seconds: the region is then exactly --steps steps
  repeats = 1
  if args.min_seconds > 0:
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    actor.launch(whole(64))
    torch.cuda.synchronize(device)
    est = (time.perf_counter() - t0) / 64
    repeats = max(1, int(np.ceil(args.min_seconds / max(1e-6, est * args.steps))))
    repeats = min(repeats, max(1, 200000 // max(1, args.steps)))
  if dist is not None:
    rt = torch.tensor([repeats], dtype=torch.int64, device=ctrl_dev)
    dist.all_reduce(rt, op=dist.ReduceOp.MAX, group=ctrl)
    repeats = int(rt.item())
  per_run = repeats * whole(args.steps)
  n_runs = max(1, args.runs) if not child else 1
  total = n_runs * per_run
  # the weight pull (storage -> [broadcast ->] repack) fires inside every timed region whatever --steps is
  sync_every = actor.config.weight_sync_frequency = max(chunk, min(sync_every, max(chunk, per_run // 2)))
  actor.launch(whole(max(args.warmup, 64 if not child and not args.envs else 0)))      # --warmup, at least 64 moves: the regions start in steady state
  pulls0 = actor.weight_pulls
  last_records = []
  if args.dump_outputs and rank == 0:
    # the records of the newest chunk the timed regions hand over (one move of B environments: its last row is kept)
    def keep_last(v):
      last_records[:] = [v[-1].copy()]
    actor.record_tap = keep_last
  runs = timed_regions(actor, layout, per_run, n_runs)
  actor.record_tap = None
  if args.dump_outputs and rank == 0:
    dump_outputs(args.dump_outputs, last_records[0], ram)
  frames = sum(r[0] for r in runs)
  dt = sum(r[1] for r in runs)
  host_cores_busy = float(np.mean([r[2] for r in runs]))
  host_cores_busy_max = float(np.max([r[3] for r in runs]))
  host_cores_busy_sum = float(np.mean([r[4] for r in runs]))
  syncs_in_region = actor.weight_pulls - pulls0 - n_runs       # (minus the forced pull that ends every Actor.launch)
  env_steps = world * B * total            # env.step() calls in the timed regions, all ranks
  run_values = [r[0] / r[1] for r in runs]
  flat = rstorage.flat if dist is not None else None
  # per rank: the frames its own replay accepted over its own clock (the per-rank-replay layout: a slow rank shows here)
  per_rank_values = [sum(r[5][k][0] for r in runs) / max(1e-9, sum(r[5][k][1] for r in runs)) for k in range(world)]
  coll_stats = None
  if dist is not None:
    torch.cuda.synchronize(device)
    mine = rstorage.collective_stats()
    every_c = [None] * world
    dist.all_gather_object(every_c, mine, group=ctrl)
    us = [c['broadcast_us'] for c in every_c if c and c.get('broadcast_us')]
    coll_stats = {'ranks_in_comm': mine['ranks_in_comm'], 'fallback_reason': next((c['fallback_reason'] for c in every_c if c and c['fallback_reason']), None),
                  'native_rccl_broadcast': all(bool(c and c['native_rccl_broadcast']) for c in every_c), 'broadcasts': mine['broadcasts'],
                  'broadcast_us': {'mean': float(np.mean([u['mean'] for u in us])), 'max': float(np.max([u['max'] for u in us])),
                                   'per_rank_mean': [c['broadcast_us']['mean'] if c and c.get('broadcast_us') else None for c in every_c],
                                   'clock': 'HIP events around mz_broadcast_weights on the side stream' if mine['native_rccl_broadcast']
                                            else 'host wall time of torch.distributed.broadcast (fallback path)'} if us else None}

  # dominant kernel = k_search_fused (one launch = all simulations of all trees of this rank + the end of the move:
  # descent, f32-MFMA dynamics + prediction, expand, backup, action/record).  Its duration is measured live with HIP
  # events on the stream it is launched on: start / stop events of every dispatch (mz_selfplay_steps_timed, the
  # timestamps rocprofv3's kernel trace reports) over a stretch of the same self-play loop, launched back to back.
  # (--full: a stretch of its own, after the timed regions)
  search_us = None
  if args.full:
    pinned = actor._pipe.pinned
    durs = []
    for _ in range(4):
      durs += eng.selfplay_steps_timed(chunk)
      eng.selfplay_drain(pinned[0], chunk)
      torch.cuda.synchronize(device)
    search_us = 1e3 * float(np.mean(durs[chunk:]))       # (first chunk = warm-up)
  # single-player shapes with their trees in LDS: the loop is ONE kernel -- every launch plays `chunk` whole moves
  # (root, simulations, end of move); mz_selfplay_steps_timed then reports every move as its share of its launch
  persistent = eng.selfplay_moves_per_launch() > 0
  moves_per_launch = min(chunk, eng.selfplay_moves_per_launch()) if persistent else 1

  # N > 1: the topology of `train --ranks N` (ONE replay on rank 0) as a secondary figure of the same line
  one_replay_secondary = None
  if args.full and dist is not None and world > 1 and not one_replay and not args.no_one_replay_secondary:
    lay2 = Layout(True, 'b')
    actor.replay_buffer = lay2.replay
    # (the ONE replay starts empty: warm up until its window has been filled once, like the priming above)
    actor.launch(whole(max(args.warmup, 64, min(int(cfg.window_size) // (B * world) + chunk, 1024))))
    r2 = timed_regions(actor, lay2, per_run, 1)[0]
    one_replay_secondary = {
        'what': 'the layout of `train --ranks N` (reference train.py:71-72: ONE replay buffer for all actors): every rank ships its '
                'record chunks through a shared-memory ring to rank 0, whose one native replay ingests them all',
        'value': r2[0] / r2[1], 'unit': 'env-steps/s', 'timed_steps': per_run, 'timed_seconds': r2[1],
        'ingest_threads_rank0': lay2.n_ingest, 'host_cores_busy_rank0': r2[2], 'host_cores_busy_max_rank': r2[3],
        'host_cores_busy_all_ranks': r2[4], 'rings': len(lay2.rings), 'rings_drained': sum(1 for r_ in lay2.rings.values() if r_.pending() == 0)}
    lay2.close()
  if publisher is not None:
    publisher.close()
  sys.stdout.flush()
  os.dup2(saved_stdout, 1)                 # stdout again: the ONE JSON line

  if rank == 0:
    value = frames / dt
    # algorithmic: SURVEY.md s8(d) per-simulation figure x sims x trees (+ the per-root figure where the root runs
    # inside the launch), x the moves one launch plays
    flops_per_launch = moves_per_launch * (SIMS * FLOP_PER_SIM + (FLOP_PER_ROOT if persistent else 0)) * B
    launch_us = search_us * moves_per_launch if search_us is not None else None
    achieved = flops_per_launch / (launch_us * 1e-6) / 1e12 if search_us is not None else None
    traffic, traffic_source = None, None
    tfile = os.path.join(ROOT, 'profiles', 'traffic.json')
    if measured_traffic is not None:
      traffic = measured_traffic['bytes_per_launch']
      traffic_source = ('measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE child passes of this command '
                        '(%d / %d launches of %d moves each), 1024 * (2 * FETCH_SIZE + WRITE_SIZE) per launch' %
                        (tuple(measured_traffic['launches']) + (moves_per_launch,)))
    elif os.path.exists(tfile) and WNAME.startswith('Lunar') and B == 4096:
      tj = json.load(open(tfile))
      tk = tj.get('k_search_fused', {})
      # (the PMC passes count per launch; a launch of the profiled command plays moves_per_launch moves)
      if 'hbm_bytes_per_move' in tk:
        traffic = tk['hbm_bytes_per_move'] * moves_per_launch
      elif moves_per_launch == 1:
        traffic = tk.get('hbm_bytes_per_launch')
      traffic_source = 'profiles/traffic.json (builder-run rocprofv3 --pmc passes of this command, %s; not re-measured ' \
                       'in this run)' % tj.get('tag', 'see file')
    if game:
      env_desc = ('TicTacToe on the device (custom_environments/tic_tac_toe.py rules; two players, known bounds (-1, 1), discount 1); ' +
                  ('whole moves inside one launch of the two-player <15,1,16> instantiation, %d moves per launch' % moves_per_launch
                   if persistent else 'one launch per step of a move, 16 moves per hipGraph'))
    else:
      env_desc = 'synthetic fixed-length episodes on the device'
    out = {
        'metric': 'env-steps/sec (self-play, whole node) at num_simulations=%d' % SIMS,
        'value': value, 'unit': 'env-steps/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': 1e3 * dt / total, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32' if not args.split_f16 else 'f16x2-split products, f32 accumulate (f32-level accuracy; secondary line)',
        'data': 'synthetic',
        'repeats': repeats, 'timed_steps': total, 'timed_seconds': dt,
        'runs': {'n': n_runs, 'values': run_values, 'mean': float(np.mean(run_values)), 'std': float(np.std(run_values)),
                 'min': float(np.min(run_values)), 'max': float(np.max(run_values)), 'steps_per_run': per_run,
                 'what': 'SURVEY.md s8(d): mean +- std of %d timed regions of %d steps each (every region bracketed by barrier + '
                         'synchronize, MAX over ranks); `value` = all frames / all seconds of the %d regions' % (n_runs, per_run, n_runs)},
        'config': {'workload': '%s shapes (obs %d%s, actions %d), FCNetwork, num_simulations=%d, '
                               '%d parallel self-play envs per GPU, synthetic fixed-length episodes T=%d, '
                               'random-init weights (torch.manual_seed(0))'
                               % (WNAME, O, ' uint8 + norm_obs 0 255' if ram else '', A, SIMS, B, EPISODE_LEN),
                   'envs_per_gpu': B, 'num_simulations': SIMS, 'episode_len': EPISODE_LEN,
                   'environment': env_desc, 'record_bytes_per_env_step': 4 * eng.rec_floats,
                   'priming': '%d untimed moves before warm-up so episode ends are in steady state' % EPISODE_LEN,
                   'timed_region': '%d regions; each = the --steps block repeated %d times back to back in one pipelined region of %.2f s '
                                   '(barrier + synchronize on both sides)' % (n_runs, repeats, dt / n_runs),
                   'sharding': 'env-id sharded, %d rank(s), weight broadcast over %s' % (world, {'nccl': 'RCCL (torch.distributed nccl backend)', None: 'nothing (one rank, no process group)'}.get(backend, backend)),
                   'replay': ('ONE native replay on rank 0 fed by every rank through shared-memory rings (--one-replay: the layout of '
                              '`train --ranks N`, reference train.py:71-72), %d ingest threads' if one_replay else
                              'one native replay per rank (bench layout: the metric counts frames accepted; `train --ranks N` merges '
                              'all ranks into ONE replay on rank 0 -- that layout is `one_replay_secondary` when N > 1; DESIGN.md s6), '
                              '%d ingest threads per rank') % layout.n_ingest,
                   'weight_sync': 'Actor.sync_weights every %d moves (storage%s -> engine repack): %d pulls inside the timed regions '
                                  '(+ the forced pull that ends each Actor.launch); a weight publisher on rank 0 stands in for '
                                  'Learner.send_weights every %.3f s; a pull waits for NOTHING queued on the GPU (mz_set_weights_async: the repack runs '
                                  'in stream order, the clamp-ReLU scale decision is made on the host copy): 0 pipeline drains'
                                  % (sync_every, ' -> broadcast of the flat f32 buffer' if dist is not None else '', syncs_in_region, args.publish_period),
                   'timed_call': 'Actor.launch(%d) per region (model-based-rl_amd/actors.py: _RecordPipe, %d-move chunks, %d pinned buffers %s; '
                                 'records logged + ingested on its worker thread); storage / replay behind rayshim handles as in train.launch'
                                 % (per_run, chunk, actor._pipe.NBUF, 'filled by a D2H copy on a copy stream (MZ_RECORD_COPY=1)' if actor._pipe.copy_stream is not None
                                    else "that the kernels' own stores fill (mz_selfplay_steps_into: `value` includes the records' way over PCIe)")},
        'env_steps_executed_per_s': env_steps / dt,
        'host_cores_busy_per_rank': host_cores_busy, 'host_cores_busy_max_rank': host_cores_busy_max,
        'host_cores_busy_all_ranks': host_cores_busy_sum, 'shards_env_ids': shards,
        'usable_host_cores': _usable_cores(), 'ingest_threads_per_rank': layout.n_ingest,
        'build_id': build_id(), 'preflight': preflight,
        'per_rank_values': per_rank_values,
        'efficiency_vs_n1': efficiency_vs_n1(frames / dt, world, one_replay),
        'collectives': {'backend': backend, 'world': world, 'forced_at_world_1': bool(force_dist and world == 1),
                        'rccl_mapped': rccl_mapped(), 'weights_on_device': bool(flat.is_cuda),
                        'ranks_in_comm': coll_stats['ranks_in_comm'], 'fallback_reason': coll_stats['fallback_reason'],
                        'native_rccl_broadcast': coll_stats['native_rccl_broadcast'], 'broadcasts': coll_stats['broadcasts'],
                        'broadcast_us': coll_stats['broadcast_us'],
                        'broadcast': 'mz_broadcast_weights: ncclBroadcast from libmz_hip.so on a side stream, step / games / scale_ok over a gloo group'
                                     if getattr(rstorage, 'native', False) else 'torch.distributed.broadcast + all_gather',
                        'what': 'broadcast of the flat f32 weights (%d floats) per pull, MAX / SUM all-reduces of the timing, '
                                'barriers' % flat.numel()} if dist is not None else None,
        'mcts_sims_per_s_per_gpu': env_steps * SIMS / dt / world,
    }
    if args.full:
      out['roofline'] = {'bound': 'mfma', 'kernel': 'k_search_fused', 'achieved': achieved,
                         'peak': PEAK_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / PEAK_F32_MFMA_TFLOPS,
                         'traffic': traffic, 'traffic_source': traffic_source,
                         'traffic_per_move': None if traffic is None else traffic / moves_per_launch, 'us_per_launch': launch_us,
                         'flop_per_launch': flops_per_launch, 'moves_per_launch': moves_per_launch,
                         'us_per_move': search_us,
                         'launch': ('one launch = %d whole moves of all trees: root (observation, initial inference, Dirichlet '
                                    'noise, first descent), %d simulations, end of move' % (moves_per_launch, SIMS)) if persistent
                                   else 'one launch = all simulations of one move of all trees + the end of the move (root: k_root)',
                         'whole_path_frac': (env_steps / dt / world) * (SIMS * FLOP_PER_SIM + FLOP_PER_ROOT) / 1e12 /
                                            PEAK_F32_MFMA_TFLOPS}
    if one_replay_secondary is not None:
      out['one_replay_secondary'] = one_replay_secondary
    if args.split_f16:
      out['secondary_line'] = True
    if args.split_f16 and args.full:
      # the split kernel executes 300 v_mfma_f32_16x16x32_f16 per wave and simulation (3 products per block, K padded to
      # 64 in the two fc1 stages): price it against the f16 matrix pipe, and show the stream that actually bounds it
      exec_flop = SIMS * B * (300 * 4 * 16384 // 16)
      stream_bytes = SIMS * (B // 16) * 21 * 8192 * 4
      out['roofline'] = {
          'bound': 'mfma', 'kernel': 'k_search_h2', 'achieved': exec_flop / (search_us * 1e-6) / 1e12, 'peak': 2516.0,
          'unit': 'TFLOP/s', 'frac': exec_flop / (search_us * 1e-6) / 1e12 / 2516.0, 'traffic': None,
          'us_per_launch': launch_us, 'flop_per_launch': exec_flop * moves_per_launch, 'moves_per_launch': moves_per_launch,
          'us_per_move': search_us, 'root_inside_the_launch': persistent,
          'algorithmic_f32_tflops': achieved, 'algorithmic_frac_of_f32_mfma_peak': achieved / PEAK_F32_MFMA_TFLOPS,
          'l2_weight_stream': {'bytes_per_launch': stream_bytes * moves_per_launch, 'achieved_TBps': stream_bytes / (search_us * 1e-6) / 1e12,
                               'peak_TBps': 39.3, 'note': '21 streamed groups x 8 KiB x 4 waves per CU and simulation; inside the '
                               'matrix stages (12.8 k of 20.8 k cycles per simulation) the stream runs at ~52 of the 64 B/clk/CU '
                               'an XCD\'s L2 delivers: that, not the matrix pipe (0.22 busy), bounds the stages (DESIGN.md s3.4)'},
          'note': 'achieved / peak = EXECUTED float16 MFMA FLOP against the dense f16 peak; the algorithmic float32 FLOP of the '
                  'same work are a third of that minus the K padding'}
    elif args.full and not args.split_f16 and world == 1 and O + 1 <= 64 and A <= 13 and not game and not child:
      # the opt-in split-f16 search kernel on the same workload, as a SECONDARY figure inside the same line (never `value`)
      try:
        with contextlib.redirect_stdout(sys.stderr):
          out['split_f16_secondary'] = measure_split_f16(device, weights, chunk)
      except Exception as exc:          # the headline must not depend on it
        out['split_f16_secondary'] = {'error': str(exc)[:200]}
    if args.policy_gain != 1.0:
      out['secondary_line'] = True
      out['config']['policy_gain'] = args.policy_gain
    if args.full and world == 1 and not args.no_depth_sensitivity and WNAME.startswith('Lunar') and not args.envs and not child and not args.split_f16 \
       and args.policy_gain == 1.0:
      try:
        with contextlib.redirect_stdout(sys.stderr):
          out['depth_sensitivity'] = depth_sensitivity(device, weights, chunk)
      except Exception as exc:          # the headline must not depend on it
        out['depth_sensitivity'] = {'error': str(exc)[:200]}
    if args.full and world == 1 and not args.no_cpu_baseline:
      out['cpu_baseline'] = cpu_baseline({k: v.numpy() for k, v in net.state_dict().items()})
      out['cpu_baseline']['reference_shaped'] = cpu_baseline_reference_shaped()
    print(json.dumps(out), flush=True)
  if dist is not None:
    barrier()
    layout.close()
    rstorage.close()
    dist.destroy_process_group()


if __name__ == '__main__':
  main()
