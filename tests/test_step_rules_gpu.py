"""GPU: a ``StepRule`` of one's own (the ancestral rule restated in tests/test_step_rules_host.py against the documented
interface) through the eager sampler on the step kernel and through ``GraphedSampler``'s captured graph."""
import pytest
import torch

from test_sa_solver_gpu import Setup
from test_step_rules_host import restated

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["mini_unet", "mini_nested"])
def test_a_rule_of_ones_own_eager_and_graphed(name):
    """batch 2, 6 steps, ddim_eta=None (rows, in-kernel generator and noise gate all in play): bit for bit solver=None on
    both paths, on a second call with other start noise through the cached graph too, in a graph entry of its own"""
    s = Setup(name)
    for call, seed in enumerate((41, 42)):
        xs = s.start(seed)
        want = s.eager(xs)
        assert torch.equal(s.eager(xs, solver=restated()), want) and torch.isfinite(want).all()
        assert torch.equal(s.graphed(xs), want) and len(s.gs._graphs) == 1 + call
        assert torch.equal(s.graphed(xs, solver=restated()), want) and len(s.gs._graphs) == 2
    assert not torch.equal(want, s.eager(xs, ddim_eta=0.0))   # the noise matters: the comparison is not vacuous
