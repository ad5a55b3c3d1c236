"""Session fixtures of the scene graph tests: the real reference's UpdateSceneGraph and the slerp oracle, compiled once (tests/scenegraph_lib.py), and the golden."""
import pytest

import native_build as nb
import scenegraph_lib as L

graph_ref = nb.ref_fixture("scenegraph_ref", L.compile_ref_shim)
graph_oracle = nb.oracle_fixture("oracle_scenegraph", L.compile_oracle)


@pytest.fixture(scope="session")
def g_graph():
    return L.golden("synthetic")


@pytest.fixture(scope="session")
def g_drone():
    return L.golden("drone")


@pytest.fixture(scope="session")
def synthetic():
    return L.synthetic()
