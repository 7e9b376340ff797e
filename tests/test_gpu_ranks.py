"""The multi-rank paths on ONE GPU: two ranks sharing it with collectives over gloo (sharding, one replay fed by two
ranks), and ONE rank with the process group over RCCL (backend "nccl", world size 1: the library is loaded, the group is
created on the device, the weights are broadcast into device memory, the all-reduces and barriers run) -- what the
driver's 8-GPU run executes, proven before an 8-GPU node shows up.  The launchers are child processes, started before
anything in them touches the GPU."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launcher(n, port):
  return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr',
          '127.0.0.1', '--master-port', str(port)]


def test_bench_two_ranks_shard_the_environments(tmp_path):
  """bench.py --gpus 2 as the driver launches it: both ranks step their own B environments, the line reports 2 ranks and
  2 x B x steps env-steps, the weight pull (broadcast + repack) fires inside the timed region, and rank 1's experience
  records equal those a single engine produces for env ids [B, 2B) -- the sharding changes nothing but who computes."""
  B, steps = 64, 16
  dump = str(tmp_path / 'rec')
  env = dict(os.environ, MZ_BENCH_BACKEND='gloo', MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
  # (regions of >= 3 s: host_cores_busy_per_rank is a steady-state figure; regions of 0.2 s are dominated by their edges --
  # barrier, synchronize, the replay's last chunk -- and read 2.0-2.1 where 3-s regions read 1.7-1.8 on the same box)
  out = subprocess.run(launcher(2, 29551) + [os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', str(steps), '--warmup',
                       '4', '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '3', '--dump-records', dump, '--full'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
  assert line['n_gpus'] == 2 and line['steps'] == steps and line['config']['envs_per_gpu'] == B
  executed = line['env_steps_executed_per_s'] * line['timed_seconds']
  assert abs(executed - 2 * B * line['timed_steps']) < 1e-6 * executed
  assert line['timed_steps'] == steps * line['repeats'] * line['runs']['n'] and line['timed_seconds'] >= 0.15
  assert line['runs']['n'] == 5 and len(line['runs']['values']) == 5 and line['runs']['std'] >= 0      # 5 runs
  # the layout of `train --ranks N` -- ONE replay on rank 0 -- rides in the same line
  o = line['one_replay_secondary']
  assert 0.6 * 2 * B * o['timed_steps'] < o['value'] * o['timed_seconds'] < 1.4 * 2 * B * o['timed_steps']
  assert line['ingest_threads_per_rank'] >= 1 and line['usable_host_cores'] >= 1
  assert 'pulls inside the timed region' in line['config']['weight_sync'] and not line['config']['weight_sync'].startswith('0 ')
  assert 0.5 * 2 * B * line['timed_steps'] < line['value'] * line['timed_seconds'] < 1.5 * 2 * B * line['timed_steps']
  assert line['collectives']['backend'] == 'gloo' and line['collectives']['world'] == 2
  assert line['host_cores_busy_per_rank'] <= 2.0, line['host_cores_busy_per_rank']       # (8 ranks fit a 16-CPU quota)
  # rank 1's records vs one engine that owns env ids [B, 2B)
  from model_based_rl_amd.engine import Engine, flatten_weights, records_view
  from model_based_rl_amd.networks import FCNetwork
  rec1 = np.load(dump + '.rank1.npy')
  rec0 = np.load(dump + '.rank0.npy')
  moves = rec1.shape[0]
  assert moves >= 16 and rec1.shape[1:] == (B, 8 + 4 + 10)
  torch.manual_seed(0)
  flat = flatten_weights(FCNetwork(8, 4, torch.device('cpu'), types.SimpleNamespace()).state_dict())
  eng = Engine(B, 8, 4, 30, seed=1234, env_id_offset=B)
  eng.set_weights(flat)
  eng.selfplay_reset(256, 1.0, stagger=True)
  eng.selfplay_steps(moves)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  one = buf[:n].numpy().copy()
  eng.close()
  assert np.array_equal(one.view(np.int32), rec1.view(np.int32))
  assert np.array_equal(records_view(rec0, 8, 4)['env_id'][0], np.arange(B))
  assert np.array_equal(records_view(rec1, 8, 4)['env_id'][0], np.arange(B, 2 * B))


def test_bench_launches_its_own_ranks():
  """`python3 bench.py --gpus 2` with no launcher (how the driver starts N = 1): bench.py starts
  torch.distributed.run as a CHILD process before touching the GPU, relays rank 0's line and the exit code."""
  B, steps = 64, 16
  env = dict(os.environ, MZ_BENCH_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
  for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
    env.pop(k, None)
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', str(steps), '--warmup', '4',
                        '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '3', '--runs', '2', '--full'],      # (3-s regions: see above)
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  rows = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(rows) == 1, out.stdout[-2000:]                   # ONE JSON line on stdout
  line = json.loads(rows[0])
  assert line['n_gpus'] == 2 and line['collectives']['world'] == 2 and line['runs']['n'] == 2
  assert 0.5 * 2 * B * line['timed_steps'] < line['value'] * line['timed_seconds'] < 1.5 * 2 * B * line['timed_steps']
  assert 'one_replay_secondary' in line and line['host_cores_busy_per_rank'] <= 2.0
  # a failing child's exit code comes back
  bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--envs', '-5',
                        '--no-cpu-baseline'], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
  assert bad.returncode != 0 and not [l for l in bad.stdout.splitlines() if l.startswith('{')]


def test_train_two_ranks_learner_broadcast_and_one_replay():
  """train --ranks 2: rank 0 = learner + storage + the one replay + actor 0, rank 1 = actor 1.  The actors run until the
  learner has reached --training_steps: its published weights travel storage -> collective broadcast -> every rank's
  engine, the training step reaches every actor, the experience of BOTH ranks lands in the one replay the learner
  samples, and the per-actor game counts come back to the storage (reference train.py:62-78, learners.py:132-133,
  actors.py:81-85,157-169)."""
  env = dict(os.environ, MZ_DIST_BACKEND='gloo', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''),
             HSA_ENABLE_IPC_MODE_LEGACY='0')
  out = subprocess.run([sys.executable, '-m', 'model_based_rl_amd.train', '--ranks', '2', '--environment', 'LunarLander-v2',
                        '--num_envs', '64', '--num_simulations', '8', '--episode_length', '6', '--max_moves', '-1',
                        '--window_size', '16384', '--stored_before_train', '1024', '--batch_size', '32',
                        '--training_steps', '6', '--send_weights_frequency', '2', '--weight_sync_frequency', '8',
                        '--seed', '3', '--use_gpu_for', 'actors', 'learner'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  s = json.loads([l for l in out.stdout.splitlines() if l.startswith('MZ_TRAIN_SUMMARY ')][-1][len('MZ_TRAIN_SUMMARY '):])
  assert s['ranks'] == 2 and s['training_step'] == 6
  assert s['rank_training_steps'] == [6, 6]                              # the learner's step reached every actor
  assert s['rank_weight_sums'][0] == s['rank_weight_sums'][1]            # ... with the same weights
  assert s['weight_broadcasts'] >= 3
  assert all(g > 0 for g in s['rank_games']) and s['actor_games'] == {'0': s['rank_games'][0], '1': s['rank_games'][1]} \
      or s['actor_games'] == {0: s['rank_games'][0], 1: s['rank_games'][1]}
  assert s['games'] == sum(s['rank_games'])                              # both ranks' games were ingested by the one replay
  assert s['frames'] >= 1024 and s['replay_size'] > 0


def test_bench_over_rccl_at_world_size_1():
  """MZ_BENCH_FORCE_DIST=1 under the launcher with ONE process: bench.py takes its multi-rank branch over backend "nccl"
  (= RCCL on ROCm): init_process_group on the device, mz_broadcast_weights of the weights INTO DEVICE MEMORY at every pull, the
  MAX / SUM all-reduces, barriers, destroy_process_group.  librccl must be mapped in the rank's process."""
  B, steps = 256, 16
  env = dict(os.environ, MZ_BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
  env.pop('MZ_BENCH_BACKEND', None)
  out = subprocess.run(launcher(1, 29561) + [os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup',
                       '4', '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '0.3', '--sync-every', '16', '--full'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  assert len(out.stdout.strip().splitlines()) == 1, out.stdout[-2000:]      # RCCL's banner and gloo's notes went to stderr: ONE line on stdout
  line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
  c = line['collectives']
  assert c['backend'] == 'nccl' and c['world'] == 1 and c['forced_at_world_1'] and c['rccl_mapped'] and c['weights_on_device']
  assert c['broadcast'].startswith('mz_broadcast_weights')            # ncclBroadcast from libmz_hip.so, on a side stream
  # what makes the first 8-GPU record self-diagnosing: RCCL's own rank count, no fallback, the broadcast's
  # HIP-event time, per-rank values, the build the line was measured on
  assert c['ranks_in_comm'] == 1 and c['fallback_reason'] is None and c['native_rccl_broadcast'] and c['broadcasts'] >= 2
  assert c['broadcast_us']['clock'].startswith('HIP events') and 0 < c['broadcast_us']['mean'] <= c['broadcast_us']['max'] < 1e5
  assert len(line['per_rank_values']) == 1 and abs(line['per_rank_values'][0] - line['value']) < 0.05 * line['value']
  assert len(line['build_id']) == 16 and line['efficiency_vs_n1'] is None and line['preflight'] is None
  assert '0 pipeline drains' in line['config']['weight_sync']
  assert line['n_gpus'] == 1 and line['metric'].startswith('env-steps/sec') and line['value'] > 0
  pulls = int(line['config']['weight_sync'].split(':')[1].split()[0])
  assert pulls >= 2, line['config']['weight_sync']                     # broadcasts of device buffers inside the timed region
  for key in ('roofline', 'ms_per_step', 'steps', 'warmup', 'scaling', 'dtype', 'config'):
    assert key in line
  assert 0.5 * B * line['timed_steps'] < line['value'] * line['timed_seconds'] < 1.5 * B * line['timed_steps']


def test_bench_falls_back_to_torch_collectives_when_the_communicator_fails():
  """The library's own RCCL communicator cannot be built (here: MZ_COMM_FAIL=1 on every rank): all ranks agree on it over the
  host-side group and the weights travel through torch.distributed's broadcast instead -- the run completes, the line says so."""
  B, steps = 256, 16
  env = dict(os.environ, MZ_BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0', MZ_COMM_FAIL='1')
  env.pop('MZ_BENCH_BACKEND', None)
  out = subprocess.run(launcher(1, 29563) + [os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup',
                       '4', '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '0.3', '--sync-every', '16', '--runs', '2'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  rows = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(rows) == 1 and len(out.stdout.strip().splitlines()) == 1, out.stdout[-2000:]      # nothing but the JSON line on stdout
  line = json.loads(rows[0])
  c = line['collectives']
  assert c['backend'] == 'nccl' and c['broadcast'].startswith('torch.distributed') and c['weights_on_device']
  assert 'falling back' in out.stderr and line['value'] > 0
  assert 'MZ_COMM_FAIL' in c['fallback_reason'] and not c['native_rccl_broadcast'] and c['ranks_in_comm'] is None      # the record says why
  assert c['broadcast_us']['clock'].startswith('host wall time')
  assert int(line['config']['weight_sync'].split(':')[1].split()[0]) >= 2


def test_train_over_rccl_at_world_size_1():
  """train --ranks 1 with the default backend: RankStorage.get_weights does its broadcast + all-gather over RCCL on device
  memory, the learner's weights and step reach the actor, the experience lands in the replay."""
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), HSA_ENABLE_IPC_MODE_LEGACY='0')
  env.pop('MZ_DIST_BACKEND', None)
  out = subprocess.run([sys.executable, '-m', 'model_based_rl_amd.train', '--ranks', '1', '--environment', 'LunarLander-v2',
                        '--num_envs', '64', '--num_simulations', '8', '--episode_length', '6', '--max_moves', '-1',
                        '--window_size', '16384', '--stored_before_train', '512', '--batch_size', '32',
                        '--training_steps', '4', '--send_weights_frequency', '2', '--weight_sync_frequency', '8',
                        '--seed', '3', '--use_gpu_for', 'actors', 'learner'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  s = json.loads([l for l in out.stdout.splitlines() if l.startswith('MZ_TRAIN_SUMMARY ')][-1][len('MZ_TRAIN_SUMMARY '):])
  assert s['backend'] == 'nccl' and s['rccl_mapped'] and s['weights_on_device'] and s['drained']
  assert s['ranks'] == 1 and s['training_step'] == 4 and s['rank_training_steps'] == [4]
  assert s['weight_broadcasts'] >= 2 and s['frames'] >= 512 and s['games'] == s['rank_games'][0]


def test_bench_two_ranks_into_one_replay():
  """bench.py --gpus 2 --one-replay: the topology of `train --ranks N` (reference train.py:71-72: ONE replay buffer) under
  the bench's clock -- rank 1 ships its record chunks through its shared-memory ring, rank 0's drain thread ingests them
  with env_base = B beside rank 0's own; the one replay accepts both ranks' frames."""
  B, steps = 64, 16
  env = dict(os.environ, MZ_BENCH_BACKEND='gloo', MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
  out = subprocess.run(launcher(2, 29571) + [os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', str(steps), '--warmup',
                       '4', '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '0.2', '--one-replay'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
  assert line['n_gpus'] == 2 and 'ONE native replay on rank 0' in line['config']['replay']
  executed = line['env_steps_executed_per_s'] * line['timed_seconds']
  assert abs(executed - 2 * B * line['timed_steps']) < 1e-6 * executed
  # frames accepted by the ONE replay = both ranks' (steady state: ~B frames per move and rank)
  assert 0.6 * 2 * B * line['timed_steps'] < line['value'] * line['timed_seconds'] < 1.4 * 2 * B * line['timed_steps']


def test_train_with_a_dedicated_learner_rank():
  """train --ranks 2 --dedicated_learner_rank: rank 0 = learner + storage + the one replay and NO actor (it only joins the
  collective weight pulls, at the actors' cadence), rank 1 = the only actor.  All experience comes through rank 1's ring,
  the learner's step and weights reach rank 1, nobody hangs in a collective."""
  env = dict(os.environ, MZ_DIST_BACKEND='gloo', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''),
             HSA_ENABLE_IPC_MODE_LEGACY='0')
  out = subprocess.run([sys.executable, '-m', 'model_based_rl_amd.train', '--ranks', '2', '--dedicated_learner_rank',
                        '--environment', 'LunarLander-v2', '--num_envs', '64', '--num_simulations', '8',
                        '--episode_length', '6', '--max_moves', '-1', '--window_size', '16384', '--stored_before_train',
                        '1024', '--batch_size', '32', '--training_steps', '6', '--send_weights_frequency', '2',
                        '--weight_sync_frequency', '8', '--seed', '3', '--use_gpu_for', 'actors', 'learner'],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  s = json.loads([l for l in out.stdout.splitlines() if l.startswith('MZ_TRAIN_SUMMARY ')][-1][len('MZ_TRAIN_SUMMARY '):])
  assert s['ranks'] == 2 and s['training_step'] == 6 and s['rank_training_steps'] == [6, 6]
  assert s['rank_weight_sums'][0] == s['rank_weight_sums'][1]
  assert s['rank_games'][0] == 0 and s['rank_games'][1] > 0 and s['games'] == s['rank_games'][1]
  assert s['frames'] >= 1024 and s['drained'] and s['dedicated_learner_rank']
  assert 'Actor-0' not in out.stdout and 'Actor-1 is online' in out.stdout


def test_bench_eight_ranks_on_one_gpu():
  """The bare `python3 bench.py --gpus 8` (the driver's N = 8 form, here with 512 environments per rank and the collectives
  over gloo: eight processes share ONE GPU) -- the only N = 8 evidence available without an 8-GPU node: bench.py launches its
  own eight ranks, every rank's Actor plays its shard of the environments (env ids [512 r, 512 (r + 1))), the weight pulls are
  collective on all eight, the ranks' host threads fit the box's cores, and the ONE-replay layout of `train --ranks 8`
  (seven shared-memory rings into rank 0's replay) keeps up with the per-rank-replay layout and drains every ring."""
  B, steps, N = 512, 16, 8
  env = dict(os.environ, MZ_BENCH_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
  for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
    env.pop(k, None)
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(N), '--steps', str(steps), '--warmup', '16',
                        '--no-cpu-baseline', '--envs', str(B), '--min-seconds', '2', '--runs', '2', '--full'],      # (regions of ~2 s: the one-replay layout starts on a fresh replay)
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  rows = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(rows) == 1, out.stdout[-2000:]
  line = json.loads(rows[0])
  assert line['n_gpus'] == N and line['collectives']['world'] == N and line['config']['envs_per_gpu'] == B
  assert line['shards_env_ids'] == [[B * r, B * (r + 1) - 1] for r in range(N)]
  executed = line['env_steps_executed_per_s'] * line['timed_seconds']
  assert abs(executed - N * B * line['timed_steps']) < 1e-6 * executed
  assert 0.6 * N * B * line['timed_steps'] < line['value'] * line['timed_seconds'] < 1.4 * N * B * line['timed_steps']
  # the host side of eight ranks fits the cores this job may use
  assert line['host_cores_busy_all_ranks'] <= line['usable_host_cores'], (line['host_cores_busy_all_ranks'], line['usable_host_cores'])
  assert line['ingest_threads_per_rank'] >= 1
  o = line['one_replay_secondary']
  assert o['rings'] == N - 1 and o['rings_drained'] == N - 1
  assert o['value'] >= 0.9 * line['value'], (o['value'], line['value'])
  assert o['host_cores_busy_all_ranks'] <= line['usable_host_cores']
  pulls = int(line['config']['weight_sync'].split(':')[1].split()[0])
  assert pulls >= 2
  # the self-diagnosing keys of an N > 1 line
  c = line['collectives']
  assert c['fallback_reason'] == 'backend gloo' and c['broadcasts'] >= 2 and len(c['broadcast_us']['per_rank_mean']) == N
  assert len(line['per_rank_values']) == N and abs(sum(line['per_rank_values']) - line['value']) < 0.25 * line['value']
  assert line['preflight']['ranks'] == N and line['preflight']['shm_need_bytes'] == (N - 1) * (64 + 4 * (8 + 16 * B * 22 * 4))
  eff = line['efficiency_vs_n1']
  assert eff is None or (eff['efficiency'] > 0 and eff['n1_file'].endswith('.json'))
  profile = os.environ.get('MZ_SAVE_PROFILE')          # (scripts/round_profile.sh keeps the line under profiles/)
  if profile:
    open(profile, 'w').write(json.dumps(line, indent=1))


def test_train_eight_ranks_with_a_dedicated_learner_rank():
  """train --ranks 8 --dedicated_learner_rank on one GPU (gloo): rank 0 = learner + storage + the one replay, ranks 1..7 = actors;
  seven rings drain, the learner's step and weights reach all eight ranks, nobody hangs in a collective."""
  N = 8
  env = dict(os.environ, MZ_DIST_BACKEND='gloo', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''),
             HSA_ENABLE_IPC_MODE_LEGACY='0')
  out = subprocess.run([sys.executable, '-m', 'model_based_rl_amd.train', '--ranks', str(N), '--dedicated_learner_rank',
                        '--environment', 'LunarLander-v2', '--num_envs', '64', '--num_simulations', '8',
                        '--episode_length', '6', '--max_moves', '-1', '--window_size', '65536', '--stored_before_train',
                        '4096', '--batch_size', '32', '--training_steps', '6', '--send_weights_frequency', '2',
                        '--weight_sync_frequency', '16', '--seed', '3', '--use_gpu_for', 'actors', 'learner'],
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  s = json.loads([l for l in out.stdout.splitlines() if l.startswith('MZ_TRAIN_SUMMARY ')][-1][len('MZ_TRAIN_SUMMARY '):])
  assert s['ranks'] == N and s['training_step'] == 6 and s['rank_training_steps'] == [6] * N
  assert len(set(s['rank_weight_sums'])) == 1
  assert s['rank_games'][0] == 0 and all(g > 0 for g in s['rank_games'][1:]) and s['games'] == sum(s['rank_games'])
  assert s['frames'] >= 4096 and s['drained'] and s['dedicated_learner_rank']
