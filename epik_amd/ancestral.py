"""Ancestral posteriors of a reference tree's ghost nodes (include/epik_amd.h, "Reconstructing ancestral posteriors").

`Ancestral` is the device handle (libepik_amd.so: epik_amd_ancestral_*), `posteriors_host` its host mirror in the
library (epik_amd_ancestral_host), `posteriors_numpy` an independent restatement of the rule in numpy: the three give
the same bytes.  `Model` reads a substitution model in RAxML-NG's notation and makes the transition matrices the rule
takes as an input (epik_amd_model_pmatrices, epik_amd_model_gamma_rates: host code, not under the bit-for-bit rule).
Model parameters are given, never optimised.
"""
from __future__ import annotations

import ctypes
import math
import re
from dataclasses import dataclass

import numpy as np

from . import alphabet, capi

#: sites a workgroup of the kernels takes (EPIK_AMD_ANCESTRAL_TILE_SITES)
TILE_SITES = 64
MAX_CATEGORIES = 8
GHOSTS = {"inner": 0, "outer": 1, "both": 2}
#: the order of the states in a PAML matrix file
PAML_STATES = "ARNDCQEGHILKMFPSTWYV"


class ModelError(ValueError):
    pass


# ---- the model ------------------------------------------------------------------------------------------------------

_HEAD = re.compile(r"^(JC|K80|HKY|GTR|POISSON|USER)(?:\{([^{}]*)\})?$")
_PART = re.compile(r"^([A-Z]+?)(\d*)(?:\{([^{}]*)\})?$")
_NUCL_MODELS = {"JC": 0, "K80": 1, "HKY": 1, "GTR": 6}


def _numbers(text, part, count, what):
    if text is None:
        raise ModelError(f"the model is incomplete: '{part}' needs {what} in braces, as in {part.split('{')[0]}{{...}}")
    try:
        values = [float(v) for v in text.split("/")]
    except ValueError:
        raise ModelError(f"'{part}': '{text}' is no list of numbers separated by '/'") from None
    if len(values) != count:
        raise ModelError(f"'{part}' needs {count} value{'s' if count != 1 else ''} ({what}), not {len(values)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in values):
        raise ModelError(f"'{part}': every value must be a finite number that is at least 0")
    return values


@dataclass
class Model:
    """A reversible substitution model with its rate heterogeneity, parameters given.

        Model.parse("GTR{1/2/1/1/2/1}+FU{0.3/0.2/0.2/0.3}+G4{0.5}+I{0.1}", "nucl")

    Substitution models: JC, K80{k}, HKY{k}, GTR{ac/ag/at/cg/ct/gt} for nucl; POISSON, or USER (the PAML-format matrix of
    `model_file`) for amino.  Frequencies: +FU{..} given, +FC counted from the alignment, +FE equal (the default of JC,
    K80 and POISSON; USER takes its file's; HKY and GTR have none and must be told).  Rates: +G4{alpha} or +Gn{alpha}
    (n categories), +I{p}.  `parse` opens no file: `resolve` reads the matrix file and counts the frequencies."""
    states: str
    name: str
    text: str
    exchange: np.ndarray | None = None      # upper triangle, row by row, in the state order of alphabet.py
    freqs: np.ndarray | None = None
    freq_mode: str = "E"                    # E equal, U given, C counted, F the matrix file's
    alpha: float | None = None
    gamma_categories: int = 0
    p_invariant: float = 0.0

    @property
    def sigma(self) -> int:
        return alphabet.alphabet_size(self.states)

    @property
    def num_categories(self) -> int:
        return max(1, self.gamma_categories) + (1 if self.p_invariant > 0.0 else 0)

    @classmethod
    def parse(cls, text: str, states: str) -> "Model":
        sigma = alphabet.alphabet_size(states)
        parts = [p.strip() for p in str(text).split("+")]
        if not parts or not parts[0]:
            raise ModelError("the model is empty: it starts with a substitution model, as in GTR{1/2/1/1/2/1}+FC+G4{0.5}")
        head = _HEAD.match(parts[0].upper())
        if not head:
            raise ModelError(f"unknown substitution model '{parts[0]}': one of JC, K80{{k}}, HKY{{k}}, GTR{{a/b/c/d/e/f}} (nucl), "
                             "POISSON, USER (amino, with --model-file)")
        name = head.group(1)
        if (name in _NUCL_MODELS) != (states == "nucl"):
            raise ModelError(f"the substitution model '{name}' is no model of -s {states}")
        model = cls(states=states, name=name, text=str(text))
        if name in _NUCL_MODELS:
            count = _NUCL_MODELS[name]
            if count == 0:
                if head.group(2) is not None:
                    raise ModelError(f"'{parts[0]}': JC has no parameter")
                model.exchange = np.ones(6)
            elif count == 1:
                k = _numbers(head.group(2), parts[0], 1, "the transition/transversion ratio")[0]
                model.exchange = np.array([1.0, k, 1.0, 1.0, k, 1.0])     # AC AG AT CG CT GT
            else:
                model.exchange = np.array(_numbers(head.group(2), parts[0], 6, "the rates ac/ag/at/cg/ct/gt"))
            if not model.exchange.any():
                raise ModelError(f"'{parts[0]}': every rate is 0")
            model.freq_mode = "E" if name in ("JC", "K80") else ""
        else:
            if head.group(2) is not None:
                raise ModelError(f"'{parts[0]}': {name} has no parameter")
            model.exchange = np.ones(190) if name == "POISSON" else None
            model.freq_mode = "E" if name == "POISSON" else "F"
        seen = set()
        for part in parts[1:]:
            m = _PART.match(part.upper())
            kind = m.group(1) if m else None
            if kind in ("FU", "FC", "FE"):
                key = "F"
            elif kind in ("G", "I"):
                key = kind
            else:
                raise ModelError(f"unknown part '+{part}' of the model: one of +FU{{..}}, +FC, +FE, +G4{{alpha}}, +Gn{{alpha}}, +I{{p}}")
            if key in seen:
                raise ModelError(f"the part '+{part}' repeats an earlier one")
            seen.add(key)
            if key == "F":
                if m.group(2):
                    raise ModelError(f"unknown part '+{part}' of the model")
                model.freq_mode = kind[1]
                if kind == "FU":
                    freqs = np.array(_numbers(m.group(3), "+" + part, sigma, f"the {sigma} frequencies"))
                    if not (freqs > 0).all():
                        raise ModelError(f"'+{part}': every frequency must be above 0")
                    model.freqs = freqs / freqs.sum()
                elif m.group(3) is not None:
                    raise ModelError(f"'+{part}': +{kind} takes no values")
            elif key == "G":
                model.gamma_categories = int(m.group(2)) if m.group(2) else 4
                if not 1 <= model.gamma_categories <= MAX_CATEGORIES:
                    raise ModelError(f"'+{part}': the number of categories must lie in [1, {MAX_CATEGORIES}]")
                model.alpha = _numbers(m.group(3), "+" + part, 1, "alpha")[0]
                if not model.alpha > 0.0:
                    raise ModelError(f"'+{part}': alpha must be above 0")
            else:
                if m.group(2):
                    raise ModelError(f"unknown part '+{part}' of the model")
                model.p_invariant = _numbers(m.group(3), "+" + part, 1, "the proportion of invariant sites")[0]
                if not model.p_invariant < 1.0:
                    raise ModelError(f"'+{part}': the proportion of invariant sites must be below 1")
        if model.freq_mode == "":
            raise ModelError(f"the model is incomplete: {name} needs its frequencies, one of +FU{{a/c/g/t}}, +FC, +FE")
        if model.num_categories > MAX_CATEGORIES:
            raise ModelError(f"the model has {model.num_categories} rate categories with +I; at most {MAX_CATEGORIES} fit")
        return model

    def check_model_file(self, model_file) -> None:
        """What can be said of --model-file before it is opened."""
        if self.name == "USER" and not model_file:
            raise ModelError("the substitution model USER needs --model-file, a matrix in PAML format")
        if self.name != "USER" and model_file:
            raise ModelError(f"--model-file goes with the substitution model USER, not with '{self.name}'")

    def resolve(self, model_file=None, masks=None) -> "Model":
        """Reads the matrix file (USER) and counts the frequencies (+FC) from the leaves' masks."""
        self.check_model_file(model_file)
        if self.name == "USER":
            exchange, freqs = read_paml_matrix(model_file)
            self.exchange = exchange
            if self.freq_mode == "F":
                self.freqs = freqs
        if self.freq_mode == "E":
            self.freqs = np.full(self.sigma, 1.0 / self.sigma)
        elif self.freq_mode == "C":
            if masks is None:
                raise ModelError("+FC needs the alignment")
            masks = np.asarray(masks, dtype=np.uint32)
            counts = np.array([np.count_nonzero(masks == np.uint32(1 << x)) for x in range(self.sigma)], dtype=np.float64)
            if not (counts > 0).all():
                missing = alphabet.state_chars(self.states)[int(np.flatnonzero(counts == 0)[0])]
                raise ModelError(f"+FC: the alignment has no unambiguous '{missing}', so its frequency would be 0; give +FU or +FE")
            self.freqs = counts / counts.sum()
        return self

    def categories(self) -> tuple:
        """(rates [C], weights [C]): the gamma categories, then the invariant one."""
        if self.gamma_categories:
            rates = gamma_rates(self.alpha, self.gamma_categories)
        else:
            rates = np.ones(1)
        weights = np.full(rates.shape[0], 1.0 / rates.shape[0])
        p = self.p_invariant
        if p > 0.0:
            rates = np.concatenate([rates / (1.0 - p), [0.0]])
            weights = np.concatenate([weights * (1.0 - p), [p]])
        return rates, weights

    def pmatrices(self, times) -> np.ndarray:
        """P(t) for every t of `times`: double [..., sigma, sigma]."""
        if self.exchange is None or self.freqs is None:
            raise ModelError("the model is not resolved: call resolve() first")
        return pmatrices(self.exchange, self.freqs, times)

    def tables(self, tree) -> tuple:
        """(weights [C], p_full, p_half, p_pend [N - 1][C][sigma][sigma]) of a newick.Tree."""
        from . import dbbuild
        rates, weights = self.categories()
        n = tree.num_nodes
        length = np.array([tree.length[b] or 0.0 for b in range(n - 1)], dtype=np.float64)
        if (length < 0).any():
            raise ModelError(f"branch {int(np.flatnonzero(length < 0)[0])} has a negative length")
        pendant = np.array(dbbuild.pendant_lengths(tree)[:n - 1], dtype=np.float64)
        full = self.pmatrices(length[:, None] * rates[None, :])
        half = self.pmatrices((length / 2.0)[:, None] * rates[None, :])
        pend = self.pmatrices(pendant[:, None] * rates[None, :])
        return weights, full, half, pend


def read_paml_matrix(path: str) -> tuple:
    """(exchangeabilities [190], frequencies [20]) in the state order of alphabet.py from a PAML-format file: the lower
    triangle row by row in PAML's order, then the 20 frequencies."""
    numbers = []
    with open(path) as fh:
        for line in fh:
            for word in line.split():
                try:
                    numbers.append(float(word))
                except ValueError:
                    break  # (a trailing comment)
            if len(numbers) >= 210:
                break
    if len(numbers) < 210:
        raise ModelError(f"{path}: {len(numbers)} numbers, a PAML matrix has 190 exchangeabilities and 20 frequencies")
    full = np.zeros((20, 20))
    at = 0
    for i in range(1, 20):
        for j in range(i):
            full[i, j] = full[j, i] = numbers[at]
            at += 1
    freqs = np.array(numbers[190:210])
    if not (np.isfinite(full).all() and (full >= 0).all() and (freqs > 0).all() and np.isfinite(freqs).all()):
        raise ModelError(f"{path}: exchangeabilities must be at least 0 and frequencies above 0")
    order = [PAML_STATES.index(c) for c in alphabet.AMINO_STATES]
    full = full[np.ix_(order, order)]
    freqs = freqs[order]
    return full[np.triu_indices(20, 1)].copy(), freqs / freqs.sum()


def pmatrices(exchange, freqs, times) -> np.ndarray:
    lib = capi.load()
    exchange = np.ascontiguousarray(exchange, dtype=np.float64)
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    shape = np.shape(times)
    times = np.ascontiguousarray(times, dtype=np.float64)
    sigma = freqs.shape[0]
    if exchange.shape != (sigma * (sigma - 1) // 2,):
        raise ValueError(f"{sigma} states have {sigma * (sigma - 1) // 2} exchangeabilities, not {exchange.shape}")
    out = np.zeros(shape + (sigma, sigma), dtype=np.float64)
    capi.check(lib.epik_amd_model_pmatrices(sigma, exchange.ctypes.data, freqs.ctypes.data, times.ctypes.data, times.size, out.ctypes.data))
    return out


def gamma_rates(alpha: float, categories: int) -> np.ndarray:
    lib = capi.load()
    out = np.zeros(max(int(categories), 0), dtype=np.float64)
    capi.check(lib.epik_amd_model_gamma_rates(float(alpha), int(categories), out.ctypes.data))
    return out


# ---- the inputs of the rule -------------------------------------------------------------------------------------------

def tree_parent(tree) -> np.ndarray:
    """parent int32 [N] of a newick.Tree (the root's is -1)."""
    return np.array(tree.parent, dtype=np.int32)


def leaf_masks(tree, by_name: dict, states: str, columns=None) -> np.ndarray:
    """uint32 [leaves][L]: per leaf of `tree`, in the order of node ids, the state masks of its sequence's `columns`."""
    table = alphabet.char_class_table(states)
    rows = []
    for leaf in tree.leaves():
        seq = np.frombuffer(by_name[tree.label[leaf]].encode("latin-1"), dtype=np.uint8)
        if columns is not None:
            seq = seq[np.asarray(columns, dtype=np.int64)]
        rows.append(table[seq])
    return np.ascontiguousarray(np.stack(rows), dtype=np.uint32)


class _Inputs:
    """The arrays of a descriptor, kept alive beside it."""

    def __init__(self, parent, sigma, weights, pi, p_full, p_half, p_pend):
        self.parent = np.ascontiguousarray(parent, dtype=np.int32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.pi = np.ascontiguousarray(pi, dtype=np.float64)
        n, c, s = self.parent.shape[0], self.weights.shape[0], int(sigma)
        self.tables = [np.ascontiguousarray(t, dtype=np.float64) for t in (p_full, p_half, p_pend)]
        for name, t in zip(("p_full", "p_half", "p_pend"), self.tables):
            if t.shape != (max(n - 1, 0), c, s, s):
                raise ValueError(f"{name} must be [{n - 1}][{c}][{s}][{s}], not {t.shape}")
        if self.pi.shape != (s,):
            raise ValueError(f"pi must be [{s}], not {self.pi.shape}")
        self.num_nodes, self.sigma, self.num_categories = n, s, c
        self.num_leaves = n - len(set(int(p) for p in self.parent if p >= 0))
        self.desc = capi.AncestralDesc(n, s, c, 0, self.parent.ctypes.data, self.weights.ctypes.data, self.pi.ctypes.data,
                                       *(t.ctypes.data for t in self.tables))

    def masks(self, masks):
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        if masks.ndim != 2 or masks.shape[0] != self.num_leaves:
            raise ValueError(f"masks must be [{self.num_leaves}][L], a row per leaf, not {masks.shape}")
        return masks

    def ghost_count(self, ghosts: int) -> int:
        return (self.num_nodes - 1) * (2 if ghosts == GHOSTS["both"] else 1)


def _ghosts(ghosts) -> int:
    if isinstance(ghosts, str):
        if ghosts not in GHOSTS:
            raise ValueError(f"ghosts must be one of {', '.join(GHOSTS)}, not '{ghosts}'")
        return GHOSTS[ghosts]
    return int(ghosts)


class Ancestral:
    """The device handle: the tree and the model's tables in, posteriors of the ghost nodes out.

        with Ancestral(parent, 4, weights, pi, p_full, p_half, p_pend) as a:
            post, branch_of, dead = a.posteriors(masks, "both")     # float32 [G][L][sigma], uint32 [G]
    """

    def __init__(self, parent, sigma, weights, pi, p_full, p_half, p_pend, device: int = 0, workspace_bytes: int = 0):
        self._lib = capi.load()
        self._in = _Inputs(parent, sigma, weights, pi, p_full, p_half, p_pend)
        self.dead_sites = 0
        handle = ctypes.c_void_p()
        capi.check(self._lib.epik_amd_ancestral_create(int(device), ctypes.byref(self._in.desc), int(workspace_bytes), ctypes.byref(handle)))
        self._handle = handle

    def posteriors(self, masks, ghosts="both") -> tuple:
        ghosts, masks = _ghosts(ghosts), self._in.masks(masks)
        G = self._in.ghost_count(ghosts) if ghosts in GHOSTS.values() else 1
        post = np.zeros((G, masks.shape[1], self._in.sigma), dtype=np.float32)
        branch_of = np.zeros(G, dtype=np.uint32)
        dead = ctypes.c_uint64()
        capi.check(self._lib.epik_amd_ancestral_posteriors(self._handle, masks.ctypes.data, masks.shape[1], ghosts, post.ctypes.data,
                                                           branch_of.ctypes.data, ctypes.byref(dead)))
        self.dead_sites = int(dead.value)
        return post, branch_of, self.dead_sites

    def posteriors_device(self, masks, ghosts="both", out=None) -> tuple:
        """The same, left on the handle's device: torch tensors float32 [G][L][sigma] and int32 [G] (the bits of uint32).
        `out`: a contiguous float32 tensor of that shape on the device to write into (made when None)."""
        import torch
        ghosts, masks = _ghosts(ghosts), self._in.masks(masks)
        G = self._in.ghost_count(ghosts) if ghosts in GHOSTS.values() else 1
        shape = (G, masks.shape[1], self._in.sigma)
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of {shape} on the device")
        d_post = torch.zeros(shape, dtype=torch.float32, device="cuda") if out is None else out
        d_branch_of = torch.zeros(G, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dead = ctypes.c_uint64()
        capi.check(self._lib.epik_amd_ancestral_posteriors_device(self._handle, masks.ctypes.data, masks.shape[1], ghosts, d_post.data_ptr(),
                                                                  d_branch_of.data_ptr(), ctypes.byref(dead)))
        self.dead_sites = int(dead.value)
        return d_post, d_branch_of, self.dead_sites

    def close(self) -> None:
        if self._handle:
            self._lib.epik_amd_ancestral_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def posteriors_host(parent, sigma, weights, pi, p_full, p_half, p_pend, masks, ghosts="both", num_threads: int = 1) -> tuple:
    """The rule on the host (epik_amd_ancestral_host): no device."""
    lib = capi.load()
    inputs = _Inputs(parent, sigma, weights, pi, p_full, p_half, p_pend)
    ghosts, masks = _ghosts(ghosts), inputs.masks(masks)
    G = inputs.ghost_count(ghosts) if ghosts in GHOSTS.values() else 1
    post = np.zeros((G, masks.shape[1], inputs.sigma), dtype=np.float32)
    branch_of = np.zeros(G, dtype=np.uint32)
    dead = ctypes.c_uint64()
    capi.check(lib.epik_amd_ancestral_host(ctypes.byref(inputs.desc), masks.ctypes.data, masks.shape[1], ghosts, int(num_threads),
                                           post.ctypes.data, branch_of.ctypes.data, ctypes.byref(dead)))
    return post, branch_of, int(dead.value)


# ---- the rule restated ------------------------------------------------------------------------------------------------

def _apply(P, v):
    """[L][C][S]: per site and category sum over y of P[c][x][y] * v[l][c][y], from the first term."""
    acc = P[None, :, :, 0] * v[:, :, None, 0]
    for y in range(1, P.shape[2]):
        acc = acc + P[None, :, :, y] * v[:, :, None, y]
    return acc


def _rescale(e):
    m = e.reshape(e.shape[0], -1).max(axis=1)
    _, exponent = np.frexp(m)
    exponent = np.where(m > 0, exponent, 0)
    return np.ldexp(e, -exponent[:, None, None])


def _row(num, rounded=True):
    Z = num[:, 0].copy()
    for x in range(1, num.shape[1]):
        Z = Z + num[:, x]
    alive = (Z > 0) & np.isfinite(Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = num / Z[:, None]
    return np.where(alive[:, None], p, 0.0).astype(np.float32 if rounded else np.float64), int((~alive).sum())


def posteriors_numpy(parent, sigma, weights, pi, p_full, p_half, p_pend, masks, ghosts="both", rounded: bool = True) -> tuple:
    """The rule restated over whole columns of sites: (post float32 [G][L][sigma], branch_of uint32 [G], dead rows).
    rounded=False leaves out the last step, the rounding to float32 (tests against sums in double)."""
    parent = np.asarray(parent, dtype=np.int64)
    weights, pi = np.asarray(weights, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    p_full, p_half, p_pend = (np.asarray(t, dtype=np.float64) for t in (p_full, p_half, p_pend))
    masks = np.asarray(masks, dtype=np.uint32)
    ghosts = _ghosts(ghosts)
    N, S, C, L = parent.shape[0], int(sigma), weights.shape[0], masks.shape[1]
    children = [[] for _ in range(N)]
    for v in range(N - 1):
        children[parent[v]].append(v)
    full_mask = np.uint32((1 << S) - 1)
    D, U, row = {}, {}, 0
    for v in range(N):                              # post-order: children first
        if not children[v]:
            m = masks[row] & full_mask
            m = np.where(m == 0, full_mask, m)
            bits = ((m[:, None] >> np.arange(S, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.float64)
            D[v] = np.broadcast_to(bits[:, None, :], (L, C, S))
            row += 1
        else:
            l, r = children[v]
            D[v] = _rescale(_apply(p_full[l], D[l]) * _apply(p_full[r], D[r]))
    for v in range(N - 2, -1, -1):                  # pre-order: parents first
        p = parent[v]
        sibling = [c for c in children[p] if c != v][0]
        f = _apply(p_full[sibling], D[sibling])
        U[v] = _rescale(f if p == N - 1 else f * _apply(p_full[p], U[p]))
    inner, outer = ghosts != GHOSTS["outer"], ghosts != GHOSTS["inner"]
    G = (N - 1) * (2 if ghosts == GHOSTS["both"] else 1)
    post = np.zeros((G, L, S), dtype=np.float32 if rounded else np.float64)
    dead = 0
    for b in range(N - 1):
        T = pi[None, None, :] * (_apply(p_half[b], D[b]) * _apply(p_half[b], U[b]))
        if inner:
            num = weights[0] * T[:, 0, :]
            for c in range(1, C):
                num = num + weights[c] * T[:, c, :]
            post[b], zeroed = _row(num, rounded)
            dead += zeroed
        if outer:
            q = p_pend[b]
            B = T[:, :, 0, None] * q[None, :, 0, :]
            for x in range(1, S):
                B = B + T[:, :, x, None] * q[None, :, x, :]
            num = weights[0] * B[:, 0, :]
            for c in range(1, C):
                num = num + weights[c] * B[:, c, :]
            post[(N - 1 if ghosts == GHOSTS["both"] else 0) + b], zeroed = _row(num, rounded)
            dead += zeroed
    branch_of = (np.arange(G) % (N - 1)).astype(np.uint32)
    return post, branch_of, dead
