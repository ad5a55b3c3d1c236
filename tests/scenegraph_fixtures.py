"""Session fixtures of the scene graph tests: the real reference's UpdateSceneGraph and the slerp oracle, compiled once (tests/scenegraph_lib.py), and the golden."""
import pytest

import scenegraph_lib as L


@pytest.fixture(scope="session")
def graph_ref(tmp_path_factory):
    r = L.compile_ref_shim(tmp_path_factory.mktemp("scenegraph_ref"))
    if r is None:
        pytest.skip("the reference checkout (TBVH_REFERENCE) is absent")
    return r


@pytest.fixture(scope="session")
def graph_oracle(tmp_path_factory):
    return L.compile_oracle(tmp_path_factory.mktemp("oracle_scenegraph"))


@pytest.fixture(scope="session")
def g_graph():
    return L.golden("synthetic")


@pytest.fixture(scope="session")
def g_drone():
    return L.golden("drone")


@pytest.fixture(scope="session")
def synthetic():
    return L.synthetic()
