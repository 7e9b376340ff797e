"""The learner step after its plan and kernels moved into one place (csrc/mz_fcl_plan.inc, fcl_kernels) computes what it computed
before, bit for bit: per step case two updates of a fixed seeded batch through mz_fcl_step, and the SHA-256 of the flat weights,
both optimiser buffers, the step counters, the new errors and the loss sums equals the digest recorded at the commit before
(tests/golden/fcl_plan_sha256.json: recorded twice there, in separate processes, with equal digests; tests/fcl_plan_util.py says
how).  The cases are the smallest batches that reach each form of the step, crossed thinly with the action counts of both
instantiations of the transition's input, the five optimiser kinds, both loss forms and clipping, so that every kernel the resolver
can return is launched (tests/test_fcl_plan_cpu.py asserts that).  Every handle's plan equals mz_fcl_plan_host at the device's CU
count."""
import json
import os

import pytest

from tests import fcl_plan_util as u

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
  from model_based_rl_amd import _abi
  return _abi.load()


@pytest.fixture(scope='module')
def golden():
  with open(os.path.join(u.GOLDEN, 'fcl_plan_sha256.json')) as f:
    return json.load(f)


@pytest.mark.parametrize('case', u.step_cases(), ids=u.step_key)
def test_two_updates_equal_the_digest_recorded_before_the_plan(lib, golden, case):
  import torch
  cus = torch.cuda.get_device_properties(0).multi_processor_count

  def check_plan(handle, shape, env, ok, sc):
    assert u.plan_of(lib, handle, ok, sc) == u.plan_host(lib, *shape, cus, env, ok, sc)
  assert u.run_step_case(lib, case, check_plan=check_plan) == golden[u.step_key(case)]
