"""The ancestral reconstruction without a device (include/epik_amd.h, "Reconstructing ancestral posteriors"): the numpy
restatement and the host mirror against a sum over all joint states of the extended tree, ghost leaves included; host
mirror bytes against numpy bytes on every case of test_ancestral_gpu.py; the model side (transition matrices, gamma
rates); the root's position; `epik.py reconstruct` tied to `epik.py build` through the files it writes, and its refusals."""
import math
import os
import re
import sys

import numpy as np
import pytest
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epik_amd import alphabet, ancestral, capi, dbbuild, newick  # noqa: E402

EPIK_PY = os.path.join(ROOT, "epik.py")
GTR = "GTR{1.3/4.1/0.7/1.1/5.2/1.0}+FU{0.31/0.19/0.22/0.28}"
SMALL_MODEL = GTR + "+G4{0.6}+I{0.15}"
SMALL_TREES = {
    "leaves2": "(a:0.13,b:0.31);",
    "leaves3": "((a:0.11,b:0.23):0.07,c:0.4);",
    "leaves4": "((a:0.11,b:0.23):0.07,(c:0.4,d:0.05):0.19);",
}
SMALL_ROWS = {"a": "ACGTNR-ACGTYA?", "b": "ACGAACGTC-TKAC", "c": "AGGTCCWTTGT-AG", "d": "TCGTACGMAGTCA."}


def load_epik_py():
    import importlib.util
    spec = importlib.util.spec_from_file_location("epik_launcher", EPIK_PY)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


# ---- cases, shared with test_ancestral_gpu.py --------------------------------------------------------------------------

def caterpillar_newick(leaves: int, length: float) -> str:
    text = f"(l0:{length},l1:{length})"
    for i in range(2, leaves):
        text = f"({text}:{length},l{i}:{length})"
    return text + ";"


def balanced_newick(depth: int, rng, zero_share: float = 0.0) -> str:
    count = [0]

    def length():
        return 0.0 if rng.random() < zero_share else float(rng.uniform(0.01, 0.4))

    def node(d):
        if d == 0:
            count[0] += 1
            return f"l{count[0] - 1}:{length()}"
        return f"({node(d - 1)},{node(d - 1)}):{length()}"
    return f"({node(depth - 1)},{node(depth - 1)});"


def random_newick(leaves: int, rng) -> str:
    parts = [f"l{i}" for i in range(leaves)]
    while len(parts) > 2:
        i, j = sorted(rng.choice(len(parts), size=2, replace=False))
        b = parts.pop(j)
        a = parts.pop(i)
        parts.append(f"({a}:{rng.uniform(0.01, 0.5):.4f},{b}:{rng.uniform(0.01, 0.5):.4f})")
    return f"({parts[0]}:{rng.uniform(0.01, 0.5):.4f},{parts[1]}:{rng.uniform(0.01, 0.5):.4f});"


def random_rows(tree, L, rng, letters, odd, odd_share=0.1):
    rows = {}
    for leaf in tree.leaves():
        seq = rng.choice(list(letters), size=L)
        swap = rng.random(L) < odd_share
        seq[swap] = rng.choice(list(odd), size=int(swap.sum()))
        rows[tree.label[leaf]] = "".join(seq)
    return rows


def inputs_of(tree, rows, model_text, states):
    """(the rule's inputs up to p_pend, masks, the resolved model)."""
    masks = ancestral.leaf_masks(tree, rows, states)
    model = ancestral.Model.parse(model_text, states).resolve(None, masks)
    weights, p_full, p_half, p_pend = model.tables(tree)
    return (ancestral.tree_parent(tree), model.sigma, weights, model.freqs, p_full, p_half, p_pend), masks, model


def _small(name):
    tree = newick.parse(SMALL_TREES[name])
    return tree, SMALL_ROWS, SMALL_MODEL, "nucl"


def _tiles(L):
    def make():
        rng = np.random.default_rng(100 + L)
        tree = newick.parse(random_newick(5, rng))
        return tree, random_rows(tree, L, rng, "ACGT", "-NRYKMSW"), GTR + "+G4{0.8}", "nucl"
    return make


def _categories(model_text):
    def make():
        rng = np.random.default_rng(7)
        tree = newick.parse(random_newick(6, rng))
        return tree, random_rows(tree, 70, rng, "ACGT", "-NRY"), model_text, "nucl"
    return make


def _amino(model_text="POISSON+G4{0.7}"):
    def make():
        rng = np.random.default_rng(11)
        tree = newick.parse(SMALL_TREES["leaves4"])
        return tree, random_rows(tree, 70, rng, alphabet.AMINO_STATES, "-XBZJ"), model_text, "amino"
    return make


def _caterpillar():
    rng = np.random.default_rng(12)
    tree = newick.parse(caterpillar_newick(700, 5.0))
    return tree, random_rows(tree, 8, rng, "ACGT", "-N", odd_share=0.02), GTR + "+G4{0.5}", "nucl"


def _balanced():
    rng = np.random.default_rng(13)
    tree = newick.parse(balanced_newick(8, rng, zero_share=0.15))
    rows = random_rows(tree, 70, rng, "ACGT", "NRYKMSWBDHV-", odd_share=0.1)
    names = sorted(rows)
    rows[names[17]] = "-" * 70                                               # an all-gap leaf
    rows = {name: seq[:33] + "-" + seq[34:] for name, seq in rows.items()}   # an all-gap column
    return tree, rows, GTR + "+G4{0.7}+I{0.05}", "nucl"


TILE = ancestral.TILE_SITES
CASES = {
    "leaves2": lambda: _small("leaves2"), "leaves3": lambda: _small("leaves3"), "leaves4": lambda: _small("leaves4"),
    f"tile-L{TILE - 1}": _tiles(TILE - 1), f"tile-L{TILE}": _tiles(TILE), f"tile-L{TILE + 1}": _tiles(TILE + 1),
    "categories-1": _categories("JC"), "categories-4": _categories("HKY{2.5}+FC+G4{1.2}"),
    "categories-8": _categories(GTR + "+G7{0.4}+I{0.2}"),
    "amino-poisson": _amino(), "amino-categories-1": _amino("POISSON"),
    "amino-categories-8": _amino("POISSON+FU{" + "/".join(str(1 + i % 4) for i in range(20)) + "}+G7{0.5}+I{0.1}"),
    "caterpillar-700": _caterpillar, "balanced-256": _balanced,
}
ALL_CASES = list(CASES)
CHUNKING_CASE = "balanced-256"
_BUILT = {}


def get_case(name):
    """dict(tree, rows, model, states, inputs, masks), built once and shared; treat as read-only."""
    if name not in _BUILT:
        tree, rows, model_text, states = CASES[name]()
        inputs, masks, model = inputs_of(tree, rows, model_text, states)
        _BUILT[name] = dict(tree=tree, rows=rows, model_text=model_text, model=model, states=states, inputs=inputs, masks=masks)
    return _BUILT[name]


_HOST = {}


def host_of(name):
    """(post, branch_of, dead) of the host mirror with both ghost nodes, computed once."""
    if name not in _HOST:
        case = get_case(name)
        _HOST[name] = ancestral.posteriors_host(*case["inputs"], case["masks"], "both", num_threads=4)
    return _HOST[name]


def same_posteriors(got, want):
    assert got[0].dtype == np.float32 and got[0].shape == want[0].shape
    assert np.array_equal(got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), f"{int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum())} values differ"
    assert got[2] == want[2]


# ---- the rule against a sum over all joint states ---------------------------------------------------------------------

def joint_sum_posteriors(tree, model, masks):
    """Per branch b the posteriors of M<b> and P<b>, double [N - 1][L][sigma] each: for every category the sum, over the
    joint states of ALL other nodes of dbbuild.extended_tree (the ghost leaves among them, all gaps), of pi at the root
    times a transition probability per branch times the leaves' indicators -- one einsum over the whole tree."""
    ext = dbbuild.extended_tree(tree, inner_labels=True)
    S = model.sigma
    rates, weights = model.categories()
    leaf_row = {tree.label[leaf]: i for i, leaf in enumerate(tree.leaves())}
    full = (1 << S) - 1
    L = masks.shape[1]
    site = ext.num_nodes  # the index shared by the leaves' indicators
    by_label = {ext.label[i]: i for i in range(ext.num_nodes) if ext.label[i]}
    out = {}
    for target in [f"{kind}{b}" for b in range(tree.num_nodes - 1) for kind in "MP"]:
        joint = np.zeros((L, S))
        for rate, weight in zip(rates, weights):
            operands = [model.freqs, [ext.root]]
            for u in range(ext.num_nodes):
                if u != ext.root:
                    operands += [model.pmatrices((ext.length[u] or 0.0) * rate), [ext.parent[u], u]]
                if ext.is_leaf(u):
                    if ext.label[u] in leaf_row:
                        m = masks[leaf_row[ext.label[u]]] & full
                        m = np.where(m == 0, full, m)
                    else:
                        m = np.full(L, full)
                    operands += [((m[:, None] >> np.arange(S)[None, :]) & 1).astype(np.float64), [site, u]]
            joint += weight * np.einsum(*operands, [site, by_label[target]], optimize="greedy")
        out[target] = joint / joint.sum(axis=1, keepdims=True)
    n = tree.num_nodes - 1
    return np.stack([out[f"M{b}"] for b in range(n)] + [out[f"P{b}"] for b in range(n)])


@pytest.mark.parametrize("name", ["leaves2", "leaves3", "leaves4"])
def test_restatement_and_host_mirror_against_the_sum_over_joint_states(name):
    """1e-12 absolute: every sum is of non-negative terms, under a thousand operations a value, so the error is at most
    about a thousand times 2^-52 = 2e-13.  The host mirror's output is float32: the rounding adds at most p 2^-24."""
    case = get_case(name)
    want = joint_sum_posteriors(case["tree"], case["model"], case["masks"])
    exact, _, dead = ancestral.posteriors_numpy(*case["inputs"], case["masks"], "both", rounded=False)
    assert dead == 0 and exact.dtype == np.float64
    print(f"{name}: numpy against the joint sum, max |d| = {np.abs(exact - want).max():.3e}")
    assert np.abs(exact - want).max() <= 1e-12
    assert np.abs(want.sum(axis=2) - 1.0).max() <= 1e-12
    host = host_of(name)[0]
    print(f"{name}: host mirror against the joint sum, max |d| = {np.abs(host - want).max():.3e}")
    assert (np.abs(host - want) <= 1e-12 + want * 2.0 ** -24).all()
    # the pieces alone: inner and outer are the halves of both
    for choice, part in (("inner", host[:host.shape[0] // 2]), ("outer", host[host.shape[0] // 2:])):
        alone = ancestral.posteriors_host(*case["inputs"], case["masks"], choice)
        assert alone[0].tobytes() == part.tobytes() and np.array_equal(alone[1], np.arange(part.shape[0]))


@pytest.mark.parametrize("name", ALL_CASES)
def test_host_mirror_bytes_equal_numpy_bytes(name):
    case = get_case(name)
    same_posteriors(host_of(name), ancestral.posteriors_numpy(*case["inputs"], case["masks"], "both"))


def test_host_mirror_threads_cannot_change_a_bit():
    case = get_case("tile-L%d" % (TILE + 1))
    same_posteriors(ancestral.posteriors_host(*case["inputs"], case["masks"], "both", num_threads=1), host_of("tile-L%d" % (TILE + 1)))


def test_scaling_keeps_the_caterpillar_alive():
    """700 leaves, every branch 5.0: unscaled doubles reach exactly 0 (0.25^700); with the scaling every row is a
    distribution."""
    post, _, dead = host_of("caterpillar-700")
    assert dead == 0 and np.isfinite(post).all()
    assert np.abs(post.sum(axis=2, dtype=np.float32) - 1.0).max() <= 1e-6
    assert 0.25 ** 700 == 0.0


def test_tile_width_is_the_header_s():
    with open(os.path.join(ROOT, "include", "epik_amd.h")) as fh:
        assert int(re.search(r"#define EPIK_AMD_ANCESTRAL_TILE_SITES (\d+)u", fh.read()).group(1)) == ancestral.TILE_SITES


# ---- the root's position -------------------------------------------------------------------------------------------------

def test_root_position_leaves_the_other_branches_alone():
    """The model is reversible: sliding the root along the path between its two children changes no other branch's
    posteriors (1e-12: the same sums in another order)."""
    results = []
    for left, right in ((0.07, 0.19), (0.20, 0.06), (0.0, 0.26)):
        tree = newick.parse(f"((a:0.11,b:0.23):{left},(c:0.4,d:0.05):{right});")
        inputs, masks, _ = inputs_of(tree, SMALL_ROWS, SMALL_MODEL, "nucl")
        results.append(ancestral.posteriors_numpy(*inputs, masks, "both", rounded=False)[0])
    others = [0, 1, 3, 4, 6 + 0, 6 + 1, 6 + 3, 6 + 4]  # M and P of the leaves' branches
    for other in results[1:]:
        assert np.abs(other[others] - results[0][others]).max() <= 1e-12
    assert np.abs(results[1][2] - results[0][2]).max() > 1e-6  # the moved midpoint does change


# ---- the model side ------------------------------------------------------------------------------------------------------

MODELS = [("JC", "nucl"), ("K80{3.5}", "nucl"), ("HKY{2.0}+FU{0.4/0.1/0.2/0.3}", "nucl"), (GTR, "nucl"), ("POISSON", "amino"),
          ("POISSON+FU{" + "/".join(str(1 + i % 5) for i in range(20)) + "}", "amino")]


@pytest.mark.parametrize("text,states", MODELS)
def test_transition_matrices(text, states):
    model = ancestral.Model.parse(text, states).resolve()
    pi, S = model.freqs, model.sigma
    s, t = 0.37, 1.21
    Ps, Pt, Pst, P0, Pinf = (model.pmatrices(x) for x in (s, t, s + t, 0.0, 400.0))
    for P in (Ps, Pt, Pst):
        assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12 and (P >= 0).all()
        assert np.abs(pi[:, None] * P - (pi[:, None] * P).T).max() <= 1e-12
    assert np.abs(Ps @ Pt - Pst).max() <= 1e-12
    assert np.array_equal(P0, np.eye(S))
    assert np.abs(Pinf - pi[None, :]).max() <= 1e-12
    # one expected substitution per unit time: -sum pi_x Q_xx = 1, Q from a short step
    h = 1e-6
    Q = (model.pmatrices(h) - np.eye(S)) / h
    assert abs(-(pi * np.diag(Q)).sum() - 1.0) <= 1e-5
    shaped = model.pmatrices(np.array([[s, t], [0.0, s + t]]))
    assert shaped.shape == (2, 2, S, S) and np.array_equal(shaped[0, 1], Pt) and np.array_equal(shaped[1, 0], np.eye(S))


def test_closed_forms_of_jc_and_k80():
    t = 0.43
    P = ancestral.Model.parse("JC", "nucl").resolve().pmatrices(t)
    same, other = 0.25 + 0.75 * math.exp(-4.0 * t / 3.0), 0.25 - 0.25 * math.exp(-4.0 * t / 3.0)
    assert np.abs(P - np.where(np.eye(4, dtype=bool), same, other)).max() <= 1e-12
    kappa = 3.5
    P = ancestral.Model.parse(f"K80{{{kappa}}}", "nucl").resolve().pmatrices(t)
    # rates: transition kappa beta, transversion beta each, (kappa + 2) beta = 1 substitution per unit time at pi = 1/4
    beta = 1.0 / (kappa + 2.0)
    e1, e2 = math.exp(-4.0 * beta * t), math.exp(-2.0 * (kappa + 1.0) * beta * t)
    want = np.full((4, 4), 0.25 - 0.25 * e1)                    # transversions
    for x, y in ((0, 2), (2, 0), (1, 3), (3, 1)):               # A<->G, C<->T
        want[x, y] = 0.25 + 0.25 * e1 - 0.5 * e2
    np.fill_diagonal(want, 0.25 + 0.25 * e1 + 0.5 * e2)
    assert np.abs(P - want).max() <= 1e-12


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_gamma_rates_at_alpha_one(K):
    rates = ancestral.gamma_rates(1.0, K)
    q = [-math.log(1.0 - i / K) if i < K else math.inf for i in range(K + 1)]
    tail = [(x + 1.0) * math.exp(-x) if math.isfinite(x) else 0.0 for x in q]
    want = np.array([K * (tail[i] - tail[i + 1]) for i in range(K)])
    assert np.abs(rates - want).max() <= 1e-12
    if K == 4:
        assert abs(rates[0] - 0.136954) < 1e-6


@pytest.mark.parametrize("alpha", [0.05, 0.3, 1.0, 2.5, 40.0])
def test_gamma_rates_have_mean_one_and_increase(alpha):
    for K in (2, 4, 8):
        rates = ancestral.gamma_rates(alpha, K)
        assert abs(rates.mean() - 1.0) <= 1e-12 and (np.diff(rates) > 0).all() and (rates >= 0).all()


def test_model_side_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    linalg = pytest.importorskip("scipy.linalg")
    for alpha in (0.3, 1.0, 2.5):
        K = 4
        cuts = stats.gamma.ppf(np.arange(K + 1) / K, alpha, scale=1.0 / alpha)
        upto = stats.gamma.cdf(cuts * alpha, alpha + 1.0)
        assert np.abs(ancestral.gamma_rates(alpha, K) - K * np.diff(upto)).max() <= 1e-10
    model = ancestral.Model.parse(GTR, "nucl").resolve()
    r = np.zeros((4, 4))
    r[np.triu_indices(4, 1)] = model.exchange
    r = r + r.T
    Q = r * model.freqs[None, :]
    np.fill_diagonal(Q, -Q.sum(axis=1))
    Q /= -(model.freqs * np.diag(Q)).sum()
    assert np.abs(model.pmatrices(0.77) - linalg.expm(Q * 0.77)).max() <= 1e-12


def test_invariant_sites_are_a_category_of_rate_zero():
    model = ancestral.Model.parse("JC+G4{0.5}+I{0.2}", "nucl")
    rates, weights = model.categories()
    assert rates.shape == (5,) and rates[-1] == 0.0 and weights[-1] == 0.2
    assert abs(weights.sum() - 1.0) <= 1e-15 and abs((rates * weights).sum() - 1.0) <= 1e-12
    assert np.allclose(rates[:4] * 0.8, ancestral.gamma_rates(0.5, 4), rtol=0, atol=1e-15)


def test_paml_matrix_file(tmp_path):
    rng = np.random.default_rng(3)
    lower = rng.uniform(0.1, 5.0, size=190)
    freqs = rng.uniform(0.5, 2.0, size=20)
    freqs /= freqs.sum()
    path = tmp_path / "m.paml"
    at, lines = 0, []
    for i in range(1, 20):
        lines.append(" ".join(repr(float(v)) for v in lower[at:at + i]))
        at += i
    path.write_text("\n".join(lines) + "\n\n" + " ".join(repr(float(v)) for v in freqs) + "\n\nA R N D ... a comment\n")
    model = ancestral.Model.parse("USER+G4{1.0}", "amino").resolve(str(path))
    order = [ancestral.PAML_STATES.index(c) for c in alphabet.AMINO_STATES]
    assert np.allclose(model.freqs, freqs[order], rtol=0, atol=1e-15)
    full = np.zeros((20, 20))
    full[np.triu_indices(20, 1)] = model.exchange
    # the exchangeability of R and H (states 0 and 1 here) is PAML's of R (1) and H (8): row 8, column 1 of the lower triangle
    assert full[0, 1] == lower[8 * 7 // 2 + 1]
    P = model.pmatrices(0.5)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12
    with pytest.raises(ancestral.ModelError, match="17 numbers"):
        bad = tmp_path / "bad.paml"
        bad.write_text(" ".join(["1.0"] * 17))
        ancestral.Model.parse("USER", "amino").resolve(str(bad))


BAD_MODELS = [
    ("", "nucl", "the model is empty"),
    ("WAG", "amino", "unknown substitution model 'WAG'"),
    ("GTR{1/2/3}+FE", "nucl", r"needs 6 values \(the rates ac/ag/at/cg/ct/gt\), not 3"),
    ("GTR+FE", "nucl", "incomplete: 'GTR' needs the rates"),
    ("GTR{1/2/1/1/2/1}", "nucl", "incomplete: GTR needs its frequencies"),
    ("HKY{2}+FU{0.5/0.5}", "nucl", r"needs 4 values \(the 4 frequencies\), not 2"),
    ("K80", "nucl", "incomplete: 'K80' needs the transition/transversion ratio"),
    ("JC+G4", "nucl", r"incomplete: '\+G4' needs alpha"),
    ("JC+G9{1.0}", "nucl", r"'\+G9\{1.0\}': the number of categories must lie in \[1, 8\]"),
    ("JC+G8{1.0}+I{0.1}", "nucl", "9 rate categories"),
    ("JC+I{1.5}", "nucl", "must be below 1"),
    ("JC+R4", "nucl", r"unknown part '\+R4'"),
    ("JC+G4{0.5}+G4{0.6}", "nucl", "repeats an earlier one"),
    ("JC+G4{x}", "nucl", "is no list of numbers"),
    ("POISSON", "nucl", "is no model of -s nucl"),
    ("JC", "amino", "is no model of -s amino"),
]


@pytest.mark.parametrize("text,states,message", BAD_MODELS)
def test_bad_models_are_refused_by_name(text, states, message):
    with pytest.raises(ancestral.ModelError, match=message):
        ancestral.Model.parse(text, states)


def test_host_entry_refusals():
    case = get_case("leaves3")
    parent, sigma, weights, pi, p_full, p_half, p_pend = case["inputs"]
    masks = case["masks"]

    def refused(message, **kw):
        args = dict(parent=parent, sigma=sigma, weights=weights, pi=pi, p_full=p_full, p_half=p_half, p_pend=p_pend)
        ghosts, rows = kw.pop("ghosts", "both"), kw.pop("masks", masks)
        args.update(kw)
        with pytest.raises(capi.EpikAmdError, match=message) as info:
            ancestral.posteriors_host(masks=rows, ghosts=ghosts, **args)
        assert info.value.code == capi.ERR_INVALID

    refused(r"parent\[4\] must be -1", parent=np.array([2, 2, 4, 4, 4], dtype=np.int32))
    refused(r"parent\[2\] = 2 is not a later node", parent=np.array([2, 2, 2, 4, -1], dtype=np.int32))
    refused("more than two children", parent=np.array([4, 4, 4, 4, -1], dtype=np.int32), masks=np.zeros((4, 14), np.uint32))
    bad = p_half.copy()
    bad[1, 2, 3, 0] = np.nan
    refused(r"p_half\[1\]\[2\]\[3\]\[0\] lies outside \[0, 2\]", p_half=bad)
    bad = weights.copy()
    bad[1] = -0.5
    refused(r"weights\[1\] is not a finite number", weights=bad)
    refused("ghosts = 3 is none of", ghosts=3)
    with pytest.raises(ValueError, match=r"masks must be \[3\]\[L\]"):
        ancestral.posteriors_host(*case["inputs"], masks[:2], "both")
    with pytest.raises(capi.EpikAmdError, match="sigma = 5 is neither 4 nor 20"):
        ancestral.posteriors_host(parent, 5, weights, np.full(5, 0.2), *(np.zeros((4, 5, 5, 5)),) * 3, masks)
    lib = capi.load()
    for symbol in ("epik_amd_ancestral_create", "epik_amd_ancestral_posteriors", "epik_amd_ancestral_posteriors_device",
                   "epik_amd_ancestral_destroy", "epik_amd_ancestral_host", "epik_amd_model_pmatrices", "epik_amd_model_gamma_rates"):
        assert hasattr(lib, symbol) and symbol in capi.EXPORTS


def test_host_code_under_sanitizers():
    """A stand-alone program over ancestral.cpp built with -fsanitize=address,undefined: the rule on a tree of four
    leaves and a caterpillar, on one thread and several, the checks' refusals and the model side.  Nothing is preloaded."""
    import subprocess
    host = os.path.join(ROOT, "epik_amd", "host")
    subprocess.run(["make", "-C", host, os.path.join(ROOT, "epik_amd", "bin", "ancestral_test"), "sanitize-ancestral"], check=True,
                   stdout=subprocess.DEVNULL)
    for binary in (os.path.join(ROOT, "epik_amd", "bin", "ancestral_test"), os.path.join(ROOT, "epik_amd", "bin", "san", "ancestral_test_asan")):
        run = subprocess.run([binary], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "ancestral selftest ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


# ---- the launcher ------------------------------------------------------------------------------------------------------------

def write_reference(folder, name="balanced", leaves=12, L=40, seed=5):
    rng = np.random.default_rng(seed)
    text = random_newick(leaves, rng)
    tree = newick.parse(text)
    rows = random_rows(tree, L, rng, "ACGT", "-NRY", odd_share=0.08)
    tree_path, fasta = str(folder / f"{name}.nwk"), str(folder / f"{name}.fasta")
    with open(tree_path, "w") as fh:
        fh.write(text + "\n")
    with open(fasta, "w") as fh:
        for label, seq in rows.items():
            fh.write(f">{label}\n{seq}\n")
    return tree_path, fasta, tree, rows


@pytest.mark.parametrize("ghosts", ["both", "inner", "outer"])
def test_reconstruct_and_build_give_the_same_database(tmp_path, ghosts):
    """`reconstruct --write-ar-probs/--write-ar-tree`, then `build` on the written files (host mirrors both): the same
    .ekdb bytes as `reconstruct` wrote itself -- %.9g gives every float32 back, and the labels and the tree are what the
    reader of `build` expects."""
    tree_path, fasta, tree, _ = write_reference(tmp_path)
    runner, launcher = CliRunner(), load_epik_py()
    db, probs, ar_tree = (str(tmp_path / n) for n in ("direct.ekdb", "ar.probs", "ar.nwk"))
    run = runner.invoke(launcher.epik, ["reconstruct", "-t", tree_path, "-r", fasta, "--model", GTR + "+G4{0.7}+I{0.1}", "-s", "nucl",
                                        "-k", "6", "--omega", "1.5", "--ghosts", ghosts, "--reduction", "0.99", "--host",
                                        "--write-ar-probs", probs, "--write-ar-tree", ar_tree, "-o", db])
    assert run.exit_code == 0, run.output
    ghost_nodes = (tree.num_nodes - 1) * (2 if ghosts == "both" else 1)
    assert re.search(rf"\d+ k-mers, \d+ phylo-k-mers from {ghost_nodes} ghost nodes of {tree.num_nodes - 1} branches, 40 sites, 5 rate categories",
                     run.output)
    again = str(tmp_path / "again.ekdb")
    info = dbbuild.build_from_files(tree_path, probs, ar_tree, "nucl", 6, 1.5, again, ghosts=ghosts, host=True)
    assert info["ghost_nodes"] == ghost_nodes and info["num_entries"] > 0
    with open(db, "rb") as a, open(again, "rb") as b:
        assert a.read() == b.read()
    first = open(probs).readline().rstrip("\n").split("\t")
    assert first == ["Node", "Site", "State", "p_A", "p_C", "p_G", "p_T"]


def test_reconstruct_refusals(tmp_path):
    tree_path, fasta, tree, rows = write_reference(tmp_path)
    runner, launcher = CliRunner(), load_epik_py()
    base = ["reconstruct", "-s", "nucl", "-k", "6", "--host", "-o", str(tmp_path / "x.ekdb")]

    def refused(message, args, tree_file=tree_path, fasta_file=fasta):
        run = runner.invoke(launcher.epik, base + ["-t", tree_file, "-r", fasta_file] + args)
        assert run.exit_code == 2 and re.search(message, run.output), run.output
        assert not os.path.exists(str(tmp_path / "x.ekdb"))

    # a bad model is refused before any file is opened: the files named here do not exist
    for text, states, message in BAD_MODELS:
        if text and states == "nucl":
            refused(message, ["--model", text], tree_file="absent.nwk", fasta_file="absent.fasta")
    refused(r"'USER' is no model of -s nucl", ["--model", "USER"], tree_file="absent.nwk")
    refused(r"--model-file goes with the substitution model USER, not with 'JC'", ["--model", "JC", "--model-file", "absent.paml"],
            tree_file="absent.nwk")
    refused(r"-t: the file 'absent.nwk' does not exist", ["--model", "JC"], tree_file="absent.nwk")
    refused(r"-k must lie in \[2, 15\]", ["--model", "JC", "-k", "16"])
    refused(r"--write-ar-probs and --write-ar-tree go together", ["--model", "JC", "--write-ar-probs", str(tmp_path / "p")])
    # files that do not fit the tree
    short = str(tmp_path / "short.fasta")
    with open(short, "w") as fh:
        for label, seq in list(rows.items())[1:]:
            fh.write(f">{label}\n{seq}\n")
    refused(r"the leaf '\w+' has no sequence in", ["--model", "JC"], fasta_file=short)
    ragged = str(tmp_path / "ragged.fasta")
    with open(ragged, "w") as fh:
        for i, (label, seq) in enumerate(rows.items()):
            fh.write(f">{label}\n{seq[:-1] if i == 3 else seq}\n")
    refused(r"has 39 columns, '\w+' has 40: the reference must be an alignment", ["--model", "JC"], fasta_file=ragged)
    trifurcation = str(tmp_path / "tri.nwk")
    with open(trifurcation, "w") as fh:
        fh.write("(l0:0.1,l1:0.1,(l2:0.1,l3:0.2):0.1);\n")
    refused(r"has 3 children: the reference tree must be binary", ["--model", "JC"], tree_file=trifurcation)
    narrow = str(tmp_path / "narrow.fasta")
    with open(narrow, "w") as fh:
        for label, seq in rows.items():
            fh.write(f">{label}\n{seq[:4]}\n")
    refused(r"4 columns are kept, fewer than k = 6", ["--model", "JC"], fasta_file=narrow)
    no_t = str(tmp_path / "no_t.fasta")
    with open(no_t, "w") as fh:
        for label, seq in rows.items():
            fh.write(f">{label}\n{seq.replace('T', 'A')}\n")
    refused(r"\+FC: the alignment has no unambiguous 'T'", ["--model", "HKY{2}+FC"], fasta_file=no_t)
