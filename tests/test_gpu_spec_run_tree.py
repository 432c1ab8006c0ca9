"""tools/gl3_spec_run --branches: tries of prompt-lookup drafts verified with gl3_forward_batch_verify_tree print exactly the ids of plain greedy
decoding on the repetitive prompt of test_gpu_spec_run_host.py; --branches 1 is the tool without the option."""
import pytest

from test_gpu_spec_run_host import NEW, setup, spec_run  # noqa: F401  (setup: the module's GGUF / prompt / greedy ids fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("draft", [4, 7])
def test_branches_3_prints_the_plain_greedy_ids(setup, draft):  # noqa: F811
    path, prompt, greedy = setup
    base = spec_run(path, prompt, ["-n", str(NEW), "--draft", str(draft)])
    assert spec_run(path, prompt, ["-n", str(NEW), "--draft", str(draft), "--branches", "1"]) == base
    got, (steps, drafted, accepted, tokens) = spec_run(path, prompt, ["-n", str(NEW), "--draft", str(draft), "--branches", "3"])
    assert got == greedy and tokens == NEW
    assert 0 < accepted < drafted and steps == NEW - accepted      # drafts stand, some are rejected
