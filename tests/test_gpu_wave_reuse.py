"""GPU tests of the factor cache of the one-wavefront path (CWBL_OPT_WAVE_REUSE, k = 41..64):
the tests that tests/factor_cache_suite.py holds for its form `wave`, which also says what they
run and compare."""
import pytest

# (the suite is no test module: its asserts are rewritten, and so explained, only when asked for)
pytest.register_assert_rewrite("factor_cache_suite")
from factor_cache_suite import WAVE, suite_of  # noqa: E402

pytestmark = pytest.mark.gpu

globals().update(suite_of(WAVE))

