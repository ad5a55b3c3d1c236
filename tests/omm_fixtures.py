"""Session fixtures of the opacity-micromap bake tests: the plain-C restatement and the real reference's CreateOpacityMicroMap, compiled once
(tests/omm_lib.py)."""
import pytest

import omm_lib as O


@pytest.fixture(scope="session")
def omm_oracle(tmp_path_factory):
    return O.compile_oracle(tmp_path_factory.mktemp("oracle_omm"))


@pytest.fixture(scope="session")
def omm_ref(tmp_path_factory):
    r = O.compile_ref_shim(tmp_path_factory.mktemp("omm_ref"))
    if r is None:
        pytest.skip("the reference checkout (TBVH_REFERENCE) is absent")
    return r
