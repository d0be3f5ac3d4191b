"""GPU tests of the device graph stage's passes around the size cap: oversized components without a meta edge, the parallel
rounds followed by cut and re-labelling in one call (also under the lap-time trace), and a second problem after a cut one.
Labels and stats are compared bit for bit with the host stage, positions with a solve over the host stage's labels."""
import pytest
import torch  # noqa: F401  (before liblfr_hip.so is loaded: one HIP runtime for both)

from lfr_amd import capi, synthetic

pytestmark = pytest.mark.gpu

LABEL_STATS = ("n_tracks", "max_track_size", "n_components", "max_component_size", "n_cut_components")
CLEAN = dict(seed=99, n_images=64, n_tracks=1000)                          # no wrong matches: every component is one track
LINKED = dict(seed=311, n_images=48, n_tracks=600, eps_out=0.03)           # wrong matches link the tracks into large components
LINKED_CAP = 200


@pytest.fixture(autouse=True)
def _hand_backs_speak(monkeypatch):
    monkeypatch.setenv("LFR_TIMING", "1")               # a hand-back of the device stage to the host stage says so on stderr


def _host_and_device(g, cap, capfd):
    """Host stage and device stage under the same cap: labels and the label stats bit-identical, equal positions."""
    ph = capi.Problem(g, max_nodes_in_component=cap)
    capfd.readouterr()
    pd = capi.Problem(g, max_nodes_in_component=cap, device_graph_stage=0)
    assert "handed back to the host" not in capfd.readouterr().err      # the device stage ran: host against host would prove nothing
    for name, x, y in zip(("track", "is_root", "comp"), ph.labels(), pd.labels()):
        assert (x == y).all(), name
    for k in LABEL_STATS:
        assert ph.stats()[k] == pd.stats()[k], k
    assert pd.stats()["tracks_ms"] > 0 and pd.stats()["assemble_ms"] == 0
    a, _ = ph.solve_hip(0)
    b, _ = pd.solve_hip(0)
    assert (a == b).all()
    return ph, pd


def test_single_tracks_above_the_cap_have_nothing_to_cut(lfr_lib, capfd):
    """A cap below the longest track: components are oversized, none has a meta edge (every component is a single track), so
    the device compacts no pair, the host cuts nothing and only counts the components above the cap."""
    g = capi.Graph.from_arrays(synthetic.generate(**CLEAN))
    ph, _ = _host_and_device(g, 4, capfd)
    st = ph.stats()
    assert st["max_track_size"] > 4 and st["n_cut_components"] > 0
    assert st["n_components"] == st["n_tracks"]         # no two tracks are linked: no meta edge anywhere


@pytest.mark.parametrize("verbose", [None, "2"])
def test_rounds_then_cut_and_relabel_in_one_call(lfr_lib, monkeypatch, capfd, verbose):
    """Every connected component through the parallel rounds, in several prefix blocks, then a cap that forces real cuts and
    the second labelling; the same with the lap-time trace on (LFR_VERBOSE=2: the stage's extra event)."""
    monkeypatch.setenv("LFR_SERIAL_SEGMENT_EDGES", "0")
    monkeypatch.setenv("LFR_ROUNDS_FIRST_BLOCK", "64")
    if verbose:
        monkeypatch.setenv("LFR_VERBOSE", verbose)
    g = capi.Graph.from_arrays(synthetic.generate(**LINKED))
    ph, pd = _host_and_device(g, LINKED_CAP, capfd)
    assert pd.stats()["kruskal_rounds"] > 0
    assert ph.stats()["n_cut_components"] > 0 and ph.stats()["n_components"] > capi.Problem(g, max_nodes_in_component=10**9).stats()["n_components"]


def test_problem_without_cap_after_a_cut_one(lfr_lib, capfd):
    """A cut problem, then a second problem on the same graph without a cap: nothing of the first call survives."""
    g = capi.Graph.from_arrays(synthetic.generate(**LINKED))
    _, cut = _host_and_device(g, LINKED_CAP, capfd)
    assert cut.stats()["n_cut_components"] > 0
    _, whole = _host_and_device(g, 10**9, capfd)
    assert whole.stats()["n_cut_components"] == 0
    assert whole.stats()["n_components"] < cut.stats()["n_components"]
