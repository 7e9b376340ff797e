#!/usr/bin/env python3
"""Golden games of the reference's evaluator (TEST INFRASTRUCTURE, runs only where the reference is mounted).

Drives the UNMODIFIED reference's evaluate.Evaluator.play_game on TicTacToe with the FCNetwork of tests/golden/g1_net_ttt.npz
and records, per configuration, tests/golden/g7_eval_ttt_<name>.npz: every move's observation, legal actions, Dirichlet
draw, select_action draws (temperature 0: u = (k + 0.5) / n_ties for the k-th tied child; temperature > 0: the
random_sample np.random.choice consumed), the random opponent's choices (index among the legal actions), predicted value,
root value, child visits, search depths and the smallest top-2 score gap of the move's MCTS decisions (margin_mcts), and
every applied action with its reward and predicted reward.  The weights are named (g1_net_ttt.npz) with their SHA-256.  tests/test_gpu_evaluate.py replays these draws through
model_based_rl_amd.evaluate.Evaluator and compares move for move.

evaluate.py imports what this machine lacks -- pyglet, pyglet.gl, ray, visualize_mcts and the reference's utils (which imports
gym) -- so those names are stand-in modules in sys.modules: utils provides get_network (the reference's networks),
get_environment (the reference's TicTacToe) and set_all_seeds (utils.py:136-144 restated, without the cudnn switches, as
oracle/make_goldens.py does).  matplotlib is stubbed only if its TkAgg backend fails.  Nothing of the reference is modified:
its modules' `np` names are wrapped in recording proxies and Config.select_action is wrapped on the config instance.

Usage: python scripts/make_eval_goldens.py [outdir]     (default tests/golden; deterministic: a re-run is byte-identical)"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_goldens as mg  # noqa: E402

A, O = 9, 9
GAMES = 3
# name -> (temperature, num_simulations, apply_mcts_actions, only_prior, only_value, use_exploration_noise, random_opp, seed)
CONFIGS = {
    'mcts_t0_opp_m1': (0.0, 30, 1, 0, 0, 0, -1, 0),
    'mcts_t0_opp_p1': (0.0, 30, 1, 0, 0, 0, 1, 10),
    'temp05': (0.5, 30, 1, 0, 0, 0, -1, 20),
    'mcts_actions3': (0.0, 30, 3, 0, 0, 0, -1, 30),
    'only_prior': (0.0, 30, 1, 1, 0, 0, -1, 40),
    'only_value': (0.0, 30, 1, 0, 1, 0, -1, 50),
    'noise': (0.0, 30, 1, 0, 0, 1, None, 60),
    'sims10': (0.0, 10, 1, 0, 0, 0, -1, 70),
}


class _Recorder(object):

  def __init__(self):
    self.moves = []          # per move dict
    self.cur = None
    self.pending_root = None  # the move's root: evaluate.py:262 creates it just before the initial inference

  def new_move(self, obs):
    self.cur = dict(obs=np.asarray(obs, np.float32).reshape(-1).copy(), walk_u=[], noise=np.zeros(A), opp=[], legal=None,
                    margin=np.inf, q=[], root=self.pending_root)
    self.moves.append(self.cur)


REC = _Recorder()


class _RandomProxy(object):
  """np.random of one reference module, recording the draws the evaluator consumes"""

  def __getattr__(self, name):
    return getattr(np.random, name)

  def choice(self, a, *args, **kw):          # evaluate.py:335, the random opponent
    out = np.random.choice(a, *args, **kw)
    REC.cur['opp'].append(int(list(np.asarray(a)).index(out)))
    return out

  def dirichlet(self, alpha, *args, **kw):   # mcts.py:59, add_exploration_noise
    out = np.random.dirichlet(alpha, *args, **kw)
    REC.cur['noise'][np.asarray(REC.cur['legal'], np.int64)] = out
    return out


class _NpProxy(object):

  def __init__(self):
    self.random = _RandomProxy()

  def __getattr__(self, name):
    return getattr(np, name)


def _stand_ins():
  import importlib
  for name in ('pyglet', 'pyglet.gl', 'visualize_mcts'):
    m = types.ModuleType(name)
    m.__all__ = []
    sys.modules[name] = m
  sys.modules['pyglet'].gl = sys.modules['pyglet.gl']
  sys.modules['visualize_mcts'].write_mcts_as_png = lambda *a, **k: None
  ray = types.ModuleType('ray')
  ray.remote = lambda f: f
  sys.modules['ray'] = ray
  try:
    import matplotlib
    matplotlib.use('TkAgg')
    import matplotlib.pyplot  # noqa: F401
  except Exception:
    for name in ('matplotlib', 'matplotlib.pyplot', 'matplotlib.animation'):
      sys.modules[name] = types.ModuleType(name)
    sys.modules['matplotlib'].use = lambda *a, **k: None
    sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
    sys.modules['matplotlib'].animation = sys.modules['matplotlib.animation']
    sys.modules['matplotlib.pyplot'].style = types.SimpleNamespace(use=lambda *a, **k: None)
  ref = mg._import_reference()
  utils = types.ModuleType('utils')

  def get_environment(config):
    env = ref.TicTacToe()
    la = env.legal_actions

    def legal_actions():
      out = la()
      if REC.cur is not None and REC.cur['legal'] is None:
        REC.cur['legal'] = np.asarray(out).copy()
      return out
    env.legal_actions = legal_actions
    return env

  def get_network(config, device=None):
    return ref.networks.FCNetwork(O, A, torch.device('cpu'), config)

  utils.get_environment, utils.get_network, utils.set_all_seeds = get_environment, get_network, mg.set_all_seeds
  sys.modules['utils'] = utils
  rev = importlib.import_module('evaluate')
  rev.np = _NpProxy()
  ref.mcts.np = _NpProxy()

  class RootNode(ref.mcts.Node):      # evaluate.py's own Node name only: the tree's children stay mcts.Node
    def __init__(self, prior):
      super().__init__(prior)
      REC.pending_root = self
  rev.Node = RootNode
  return ref, rev, utils


def _weights():
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g1_net_ttt.npz'))
  return {k[2:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith('w.')}


def gen_config(ref, rev, utils, name, spec, outdir):
  temp, sims, apply_n, only_prior, only_value, noise, random_opp, seed0 = spec
  argv = ['--environment', 'TicTacToe', '--two_players', '--known_bounds', '-1', '1', '--discount', '1', '--num_simulations',
          str(sims), '--seed', str(seed0)]
  cfg = mg.make_ref_config(ref, argv, A, (O,))
  # what state_generator sets (evaluate.py:417-437)
  for k, v in dict(saves_dir='', temperature=temp, only_value=only_value, only_prior=only_prior, use_exploration_noise=noise,
                   apply_mcts_actions=apply_n, render=False, save_mcts=False, save_mcts_after_step=0, save_gif_as='', sleep=0,
                   random_opp=random_opp, human_opp=None, label=name, use_gpu=False, verbose=False).items():
    setattr(cfg, k, v)
  weights = _weights()
  ev = rev.Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  ev.mcts = mg.margin_mcts(ref, cfg)
  run_mcts = ev.mcts.run

  def run(root, network):
    ev.mcts.min_margin = float('inf')
    out = run_mcts(root, network)
    REC.cur['margin'] = ev.mcts.min_margin
    return out
  ev.mcts.run = run
  init = ev.network.initial_inference

  def initial_inference(obs):
    REC.new_move(obs.numpy())
    return init(obs)
  ev.network.initial_inference = initial_inference
  rec_inf = ev.network.recurrent_inference

  def recurrent_inference(hidden, action):
    out = rec_inf(hidden, action)
    if hidden.shape[0] == 1 and REC.cur is not None and (only_value or only_prior):   # the lookahead's rows (evaluate.py:280-294)
      q = (out.reward - cfg.discount * out.value) if cfg.two_players else (out.reward + cfg.discount * out.value)
      REC.cur['q'].append(q.item())
    return out
  ev.network.recurrent_inference = recurrent_inference

  def lookahead_margin():
    # the lookahead's decision margin: top-2 gap of the q values (only_value) or of the root priors (only_prior)
    if only_value and len(REC.cur['q']) > 1:
      v = sorted(REC.cur['q'], reverse=True)
      REC.cur['margin'] = v[0] - v[1]
    elif only_prior and REC.cur['root'] is not None and len(REC.cur['root'].children) > 1:
      v = sorted((c.prior for c in REC.cur['root'].children.values()), reverse=True)
      REC.cur['margin'] = v[0] - v[1]

  def select_action(node, temperature=0.):
    counts = np.array([c.visit_count for c in node.children.values()])
    action, u = mg.choice_uniform_and_action(ref.config.Config, node, temperature)
    if not temperature:
      ties = list(np.flatnonzero(counts == counts.max()))
      u = (ties.index(list(node.children.keys()).index(action)) + 0.5) / len(ties)
    REC.cur['walk_u'].append(u)
    return action
  cfg.select_action = select_action

  # the weights are g1_net_ttt.npz's (named, with a digest, instead of a 0.8 MB copy in every file)
  import hashlib
  digest = hashlib.sha256(b''.join(weights[k].numpy().tobytes() for k in sorted(weights))).hexdigest()
  out = {'weights_file': np.array('g1_net_ttt.npz'), 'weights_sha256': np.array(digest)}
  per_move, per_act = [], []
  seeds = list(range(seed0, seed0 + GAMES))
  game_step, game_return = [], []
  for gi, seed in enumerate(seeds):
    REC.moves, REC.cur = [], None
    game = rev.run(ev, seed)
    assert len(REC.moves) == len(game.pred_values) == len(game.history.child_visits)
    for m, rec in enumerate(REC.moves):
      REC.cur = rec
      lookahead_margin()
      d = game.search_depths[m]
      per_move.append(dict(game=gi, obs=rec['obs'], legal=np.isin(np.arange(A), rec['legal']).astype(np.uint8),
                           walk_u=rec['walk_u'], noise=rec['noise'], opp=rec['opp'], margin=rec['margin'],
                           pred_value=float(game.pred_values[m]), root_value=float(game.history.root_values[m]),
                           child_visits=np.asarray(game.history.child_visits[m], np.float64), depths=list(d)))
    for j, a in enumerate(game.history.actions):
      per_act.append(dict(game=gi, action=int(a), reward=float(game.history.rewards[j]), pred_reward=float(game.pred_rewards[j]),
                          done=bool(game.history.dones[j])))
    game_step.append(game.step)
    game_return.append(float(sum(game.history.rewards)))
  n = len(per_move)
  mw = max(1, max(len(r['walk_u']) for r in per_move))
  mo = max(1, max(len(r['opp']) for r in per_move))
  md = max(len(r['depths']) for r in per_move)
  walk_u = np.full((n, mw), -1.0); opp = np.full((n, mo), -1, np.int32); depths = np.full((n, md), -1, np.int32)
  for i, r in enumerate(per_move):
    walk_u[i, :len(r['walk_u'])] = r['walk_u']
    opp[i, :len(r['opp'])] = r['opp']
    depths[i, :len(r['depths'])] = r['depths']
  out.update(
      temperature=np.float64(temp), num_simulations=np.int32(sims), apply_mcts_actions=np.int32(apply_n),
      only_prior=np.int32(only_prior), only_value=np.int32(only_value), use_exploration_noise=np.int32(noise),
      random_opp=np.int32(0 if random_opp is None else random_opp), seeds=np.array(seeds, np.int32),
      move_game=np.array([r['game'] for r in per_move], np.int32), obs=np.stack([r['obs'] for r in per_move]),
      legal=np.stack([r['legal'] for r in per_move]), walk_u=walk_u, walk_n=np.array([len(r['walk_u']) for r in per_move], np.int32),
      noise=np.stack([r['noise'] for r in per_move]), opp=opp, opp_n=np.array([len(r['opp']) for r in per_move], np.int32),
      margin=np.array([r['margin'] for r in per_move]), pred_value=np.array([r['pred_value'] for r in per_move]),
      root_value=np.array([r['root_value'] for r in per_move]), child_visits=np.stack([r['child_visits'] for r in per_move]),
      search_depths=depths, search_depths_n=np.array([len(r['depths']) for r in per_move], np.int32),
      act_game=np.array([r['game'] for r in per_act], np.int32), action=np.array([r['action'] for r in per_act], np.int32),
      reward=np.array([r['reward'] for r in per_act]), pred_reward=np.array([r['pred_reward'] for r in per_act]),
      done=np.array([r['done'] for r in per_act], np.uint8), game_step=np.array(game_step, np.int32),
      game_return=np.array(game_return))
  path = os.path.join(outdir, 'g7_eval_ttt_%s.npz' % name)
  np.savez_compressed(path, **out)
  return path, n


def main():
  outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden')
  os.makedirs(outdir, exist_ok=True)
  ref, rev, utils = _stand_ins()
  import contextlib
  import io
  for name, spec in CONFIGS.items():
    with contextlib.redirect_stdout(io.StringIO()):        # (the reference's per-game lines)
      path, n = gen_config(ref, rev, utils, name, spec, outdir)
    print('%s: %d moves, %d bytes' % (os.path.basename(path), n, os.path.getsize(path)))


if __name__ == '__main__':
  main()
