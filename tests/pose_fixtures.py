"""Session fixtures of the pose tests: the plain-C restatement and the real reference's Mesh::SetPose, compiled once (tests/pose_lib.py)."""
import pytest

import pose_lib as P


@pytest.fixture(scope="session")
def pose_oracle(tmp_path_factory):
    return P.compile_oracle(tmp_path_factory.mktemp("oracle_pose"))


@pytest.fixture(scope="session")
def pose_ref(tmp_path_factory):
    r = P.compile_ref_shim(tmp_path_factory.mktemp("pose_ref"))
    if r is None:
        pytest.skip("the reference checkout (TBVH_REFERENCE) is absent")
    return r
