"""GPU tests of the factor cache of the hand-off path at k = 97..128 (CWBL_OPT_ROWS_REUSE):
the tests that tests/factor_cache_suite.py holds for its form `rows`, which also says what they
run and compare."""
import pytest

# (the suite is no test module: its asserts are rewritten, and so explained, only when asked for)
pytest.register_assert_rewrite("factor_cache_suite")
from factor_cache_suite import ROWS, suite_of  # noqa: E402

pytestmark = pytest.mark.gpu

globals().update(suite_of(ROWS))

