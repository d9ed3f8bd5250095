"""Taxonomy handling and hierarchical losses -- drop-in for hierarchy.py.

Host-side integer work (label parsing, tier-id assignment, parent lookup, the
leaf permutation that makes every taxonomy node a contiguous leaf range) is
plain Python/numpy and bit-exact with the reference.  The losses run as HIP
kernels (ops.multitask_cross_entropy, ops.hierarchical_cross_entropy and, for
probability targets over the leaves such as LabelSmoothing's,
ops.hierarchical_cross_entropy_soft: the expectation of the hard HXE loss, over
the rank-ordered node tables of Taxonomy.soft_tables(); ops.soft_labels_cross_entropy and
ops.soft_labels_cross_entropy_dense for the soft-labels loss, SoftLabelsCrossEntropy).
"""
import collections
import dataclasses
import math
import os
import pathlib

import numpy as np
import torch

from . import ops

N_TIERS = 7


# --------------------------------------------------------------------------- labels
@dataclasses.dataclass(frozen=True)
class HierarchicalLabel:
    """`NNNNN_kingdom_phylum_class_order_family_genus_species` with every tier
    prefixed by its ancestors so repeated names on different branches stay
    distinct (hierarchy.py:230-330)."""
    raw: str
    number: int
    kingdom: str
    phylum: str
    cls: str
    order: str
    family: str
    genus: str
    species: str

    @classmethod
    def parse(cls, name):
        index, top, *tiers = name.split("_")
        cleaned, complete = [top], top
        for tier in tiers:
            complete = f"{complete}-{tier}"
            cleaned.append(complete)
        assert len(cleaned) == N_TIERS, f"{len(cleaned)} != {N_TIERS}"
        return cls(name, int(index), *cleaned)

    @property
    def clean_tiers(self):
        return [self.kingdom, self.phylum, self.cls, self.order, self.family, self.genus,
                self.species]

    @property
    def cleaned(self):
        return "_".join([str(self.number).rjust(5, "0")] + self.clean_tiers)

    def dist(self, other: "HierarchicalLabel") -> int:
        mine, theirs = self.clean_tiers, other.clean_tiers
        for level, t in enumerate(range(N_TIERS - 1, -1, -1)):
            if mine[t] == theirs[t]:
                return level
        return N_TIERS


def assign_tier_ids(class_names):
    """Tier ids in first-seen order over sorted() names (hierarchy.py:202-227).

    Returns (classes, {class: LongTensor[7]}, num_classes tuple)."""
    classes = sorted(class_names)
    lookup = [dict() for _ in range(N_TIERS)]
    out = {}
    for c in classes:
        ids = []
        for t, v in enumerate(HierarchicalLabel.parse(c).clean_tiers):
            ids.append(lookup[t].setdefault(v, len(lookup[t])))
        out[c] = torch.tensor(ids)
    return classes, out, tuple(len(d) for d in lookup)


class HierarchicalImageFolder:
    """Only the class-indexing half of the reference's image folder
    (hierarchy.py:188-227); image decoding is outside this hot path."""

    num_classes = None

    def find_classes(self, directory):
        names = [e.name for e in os.scandir(directory) if e.is_dir()]
        classes, class_to_idxs, self.num_classes = assign_tier_ids(names)
        return classes, class_to_idxs


def _split_class_names(directory):
    directory = pathlib.Path(directory)
    train = {p.stem for p in (directory / "train").iterdir()}
    val = {p.stem for p in (directory / "val").iterdir()}
    return sorted(train | val)


def build_parent_label_lookup(directory):
    """(n_tiers - 1) uint16 vectors child id -> parent id (hierarchy.py:429-485)."""
    return parent_vectors([HierarchicalLabel.parse(n) for n in _split_class_names(directory)])


def parent_vectors(labels):
    lookups = [dict() for _ in range(N_TIERS)]
    for label in labels:
        for i, v in enumerate(label.clean_tiers):
            lookups[i].setdefault(v, len(lookups[i]))
    vecs = []
    for i in range(1, N_TIERS):
        vec = np.zeros((len(lookups[i]),), dtype=np.uint16)
        for label in labels:
            t = label.clean_tiers
            vec[lookups[i][t[i]]] = lookups[i - 1][t[i - 1]]
        vecs.append(vec)
    return vecs


def build_tree_dist_matrix(labels):
    """uint8 [n, n] tree distances (hierarchy.py:391-426) from parsed labels,
    vectorised over the 7 tier-id columns."""
    _, c2i, _ = assign_tier_ids([lb.raw for lb in labels])
    ids = np.stack([c2i[lb.raw].numpy() for lb in sorted(labels, key=lambda x: x.raw)])
    dist = np.full((len(ids), len(ids)), N_TIERS, dtype=np.uint8)
    for lvl, t in enumerate(range(N_TIERS - 1, -1, -1)):
        same = ids[:, None, t] == ids[None, :, t]
        dist = np.where(same & (dist == N_TIERS), np.uint8(lvl), dist)
    return torch.from_numpy(dist)


# --------------------------------------------------------------------------- taxonomy
class Taxonomy:
    """Leaf paths of a 7-tier taxonomy plus the segment tables the HXE kernel scans.

    leaf_paths[k] = tier ids of leaf k (leaf id = species tier id = index of
    the class in sorted() order).  ``perm`` orders leaves lexicographically by
    their path, which makes every node's leaves one contiguous range
    [node_start, node_end) of permuted positions -- for iNat21-style names
    (numbered in taxonomic order) perm is the identity."""

    def __init__(self, class_names):
        self.classes, c2i, self.num_classes = assign_tier_ids(class_names)
        self.leaf_paths = np.stack([c2i[c].numpy() for c in self.classes]).astype(np.int64)
        if self.num_classes[-1] != len(self.classes):
            raise ValueError("every class must be its own leaf (distinct species paths)")
        self.perm = np.lexsort(self.leaf_paths.T[::-1]).astype(np.int32)
        self.identity_perm = bool(np.all(self.perm == np.arange(len(self.perm))))
        ordered = self.leaf_paths[self.perm]
        starts, ends = [], []
        for t in range(N_TIERS):
            n = self.num_classes[t]
            col = ordered[:, t]
            st = np.full(n, -1, np.int64)
            en = np.full(n, -1, np.int64)
            change = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
            bounds = np.r_[change, len(col)]
            for a, b in zip(bounds[:-1], bounds[1:]):
                node = col[a]
                if st[node] != -1:
                    raise ValueError(f"tier {t} node {node} is not contiguous in path order")
                st[node], en[node] = a, b
            starts.append(st)
            ends.append(en)
        self.node_start = np.concatenate(starts).astype(np.int32)
        self.node_end = np.concatenate(ends).astype(np.int32)
        self.tier_base = np.r_[0, np.cumsum(self.num_classes)[:-1]].astype(np.int32)
        self._dev = {}
        self._soft = None
        self._soft_dev = {}
        self._backoff_dev = {}
        self._parents = None
        self._parents_dev = {}
        self._siblings = None
        self._siblings_dev = {}
        self._norms = {}

    @property
    def num_leaves(self):
        return len(self.classes)

    @classmethod
    def from_directory(cls, directory):
        return cls(_split_class_names(directory))

    @classmethod
    def synthetic(cls, sizes=(3, 13, 51, 273, 1103, 4884, 10000)):
        """iNat21-shaped synthetic tree: parent of node i at
        tier t is floor(i * n_{t-1} / n_t)."""
        n_leaves = sizes[-1]
        names = []
        for leaf in range(n_leaves):
            ids = [0] * N_TIERS
            ids[-1] = leaf
            for t in range(N_TIERS - 2, -1, -1):
                ids[t] = ids[t + 1] * sizes[t] // sizes[t + 1]
            names.append("_".join([f"{leaf:05d}"] + [f"t{t}n{ids[t]}" for t in range(N_TIERS)]))
        return cls(names)

    def device_tables(self, device):
        """(perm or None, node_start, node_end, tier_base, leaf_paths) on `device`."""
        key = str(device)
        if key not in self._dev:
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._dev[key] = (None if self.identity_perm else mk(self.perm), mk(self.node_start),
                              mk(self.node_end), mk(self.tier_base), mk(self.leaf_paths))
        return self._dev[key]

    def parent_tables(self):
        """(tier_off [8], parents) as numpy int32, built once: tier t is columns [tier_off[t],
        tier_off[t + 1]) of the concatenated tier logits, and the parent (a tier t - 1 id) of
        node n of tier t >= 1 is parents[tier_off[t] - tier_off[1] + n] (hvk_joint_decode)."""
        if self._parents is None:
            off = np.r_[0, np.cumsum(self.num_classes)].astype(np.int32)
            parents = np.full(off[-1] - off[1], -1, np.int32)
            for t in range(1, N_TIERS):
                parents[off[t] - off[1] + self.leaf_paths[:, t]] = self.leaf_paths[:, t - 1]
            if (parents < 0).any():
                raise ValueError("a tier id has no leaf below it")
            self._parents = (off, parents)
        return self._parents

    def device_parent_tables(self, device):
        """(parents int32, leaf_paths int32 [L, 7]) of parent_tables() on `device`."""
        key = str(device)
        if key not in self._parents_dev:
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._parents_dev[key] = (mk(self.parent_tables()[1]), mk(self.leaf_paths.astype(np.int32)))
        return self._parents_dev[key]

    def sibling_tables(self):
        """(sib_ptr [G + 1], sib_col [N]) as numpy int32, built once: the sibling groups of the
        conditional softmax (hvk_cond_softmax_*) as a CSR over the concatenated column space [0, N)
        of parent_tables().  G = 1 + tier_off[6] groups, the root's first, then by (parent tier,
        parent id): group 0 holds the tier-0 columns, group 1 + tier_off[t - 1] + p the columns of
        the children of node p of tier t - 1, ascending, so tier t's columns are CSR positions
        [tier_off[t], tier_off[t + 1]).  `identity_siblings`: sib_col is arange(N) (iNat21-style
        names, Taxonomy.synthetic), and the kernels are handed no sib_col at all."""
        if self._siblings is None:
            off, parents = self.parent_tables()
            group = np.zeros(off[-1], np.int64)  # a column's group, from its parent
            for t in range(1, N_TIERS):
                group[off[t]:off[t + 1]] = 1 + off[t - 1] + parents[off[t] - off[1]:off[t + 1] - off[1]]
            sib_col = np.argsort(group, kind="stable").astype(np.int32)
            sib_ptr = np.r_[0, np.cumsum(np.bincount(group, minlength=1 + off[N_TIERS - 1]))].astype(np.int32)
            self.identity_siblings = bool(np.all(sib_col == np.arange(off[-1])))
            self._siblings = (sib_ptr, sib_col)
        return self._siblings

    def device_sibling_tables(self, device):
        """(sib_ptr, sib_col or None where it is the identity) of sibling_tables() on `device`."""
        key = str(device)
        if key not in self._siblings_dev:
            sib_ptr, sib_col = self.sibling_tables()
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._siblings_dev[key] = (mk(sib_ptr), None if self.identity_siblings else mk(sib_col))
        return self._siblings_dev[key]

    def soft_tables(self):
        """The node-slot tables of the soft-target HXE kernels (numpy int32, built once).

        The internal nodes of tier t (0..5) are ranked by node_start; the node of rank r has
        slot rank_off[t] + r, the root slot n_nodes = rank_off[6] (rank_off[7] = n_nodes + 1).
        Returns (rank_off [8], child_lo, child_hi [n_nodes + 1], anc [L, 6], slot_node
        [n_nodes]): the children of slot i are [child_lo[i], child_hi[i]) -- permuted leaf
        positions for tier 5, slots of the next finer tier above it (the root's are tier 0);
        anc[p, t] is the slot of the tier-t ancestor of permuted position p; slot_node[i] is
        the tier id of the node in slot i (host side only)."""
        if self._soft is None:
            tiers = N_TIERS - 1
            rank_off = np.r_[0, np.cumsum(self.num_classes[:tiers])]
            n_nodes = int(rank_off[-1])
            rank_off = np.r_[rank_off, n_nodes + 1]
            ordered = self.leaf_paths[self.perm]
            child_lo = np.zeros(n_nodes + 1, np.int64)
            child_hi = np.zeros(n_nodes + 1, np.int64)
            anc = np.zeros((self.num_leaves, tiers), np.int64)
            slot_node = np.zeros(n_nodes, np.int64)
            finer = None  # sorted starts of the next finer tier
            for t in range(tiers - 1, -1, -1):
                n = self.num_classes[t]
                st = self.node_start[self.tier_base[t]:self.tier_base[t] + n].astype(np.int64)
                en = self.node_end[self.tier_base[t]:self.tier_base[t] + n].astype(np.int64)
                order = np.argsort(st, kind="stable")  # rank -> node id
                rank = np.empty(n, np.int64)
                rank[order] = np.arange(n)
                sl = slice(rank_off[t], rank_off[t + 1])
                slot_node[sl] = order
                if finer is None:
                    child_lo[sl], child_hi[sl] = st[order], en[order]
                else:  # ranges nest: the children are the finer nodes that start inside
                    child_lo[sl] = rank_off[t + 1] + np.searchsorted(finer, st[order])
                    child_hi[sl] = rank_off[t + 1] + np.searchsorted(finer, en[order])
                anc[:, t] = rank_off[t] + rank[ordered[:, t]]
                finer = st[order]
            child_lo[n_nodes], child_hi[n_nodes] = rank_off[0], rank_off[1]
            self._soft = tuple(a.astype(np.int32) for a in (rank_off, child_lo, child_hi, anc,
                                                             slot_node))
        return self._soft

    def device_soft_tables(self, device):
        """(perm or None, rank_off, child_lo, child_hi, anc) of soft_tables() on `device`."""
        key = str(device)
        if key not in self._soft_dev:
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._soft_dev[key] = (None if self.identity_perm else mk(self.perm),
                                   *(mk(a) for a in self.soft_tables()[:4]))
        return self._soft_dev[key]

    def device_backoff_tables(self, device):
        """(perm or None, rank_off, child_lo, child_hi, slot_node) of soft_tables() as back-off
        decoding reads them (ops.backoff_decode): everything on `device` but rank_off, which stays
        a host tensor -- the entry point sizes its LDS from it before the launch."""
        key = str(device)
        if key not in self._backoff_dev:
            mk = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            rank_off, child_lo, child_hi, _, slot_node = self.soft_tables()
            self._backoff_dev[key] = (None if self.identity_perm else mk(self.perm), torch.from_numpy(rank_off),
                                      mk(child_lo), mk(child_hi), mk(slot_node))
        return self._backoff_dev[key]

    def soft_label_norms(self, level_weights, device=None):
        """float32 [L], by leaf id: 1 / Z_c of the soft-labels loss, Z_c = sum_l w_l (|A_l(c)| -
        |A_{l-1}(c)|) over the nested leaf ranges A_0(c) = {c} .. A_7(c) = all leaves of c's
        ancestors (= sum_k w[d(c, k)]).  Computed in float64 from the node sizes; cached per
        weights and device (None: the host)."""
        w = tuple(float(x) for x in level_weights)
        if len(w) != N_TIERS + 1 or not all(math.isfinite(x) and x >= 0 for x in w) or w[0] <= 0:
            raise ValueError(f"soft-label level weights must be {N_TIERS + 1} finite non-negative "
                             f"numbers with w_0 > 0, got {w}")
        key = (w, str(device))
        if key not in self._norms:
            if (w, "None") not in self._norms:
                size = np.ones((N_TIERS + 1, self.num_leaves))  # |A_l(c)|, l = 0 the leaf itself
                for l in range(1, N_TIERS):
                    k = self.tier_base[N_TIERS - 1 - l] + self.leaf_paths[:, N_TIERS - 1 - l]
                    size[l] = self.node_end[k].astype(np.float64) - self.node_start[k]
                size[N_TIERS] = self.num_leaves
                z = np.asarray(w) @ np.diff(size, axis=0, prepend=0.0)
                self._norms[(w, "None")] = torch.from_numpy((1.0 / z).astype(np.float32))
            self._norms[key] = self._norms[(w, "None")].to(device) if device is not None \
                else self._norms[(w, "None")]
        return self._norms[key]


def soft_label_level_weights(beta):
    """w_l = exp(-beta l / 7) for tree distances l = 0 .. 7, float32 [8]: the soft-labels loss's
    target of class c is softmax_k(-beta d(c, k) / 7) (Bertinetto et al. 2020, section 3.2, with
    the distance normalised by the tree height)."""
    return torch.tensor([math.exp(-beta * l / N_TIERS) for l in range(N_TIERS + 1)],
                        dtype=torch.float32)


def hxe_level_coeffs(tree_weights="uniform", alpha=0.1):
    """Coefficients c_l of L = sum_l c_l LSE_l for levels l = 0 (leaf) .. 7 (root):
    L = -sum_{l<7} lambda_l (LSE_l - LSE_{l+1}), lambda_l = 1 (uniform) or
    exp(-alpha * l) (exponential; Bertinetto et al. 2020)."""
    if tree_weights == "uniform":
        lam = [1.0] * N_TIERS
    elif tree_weights == "exponential":
        lam = [math.exp(-alpha * l) for l in range(N_TIERS)]
    else:
        raise ValueError(tree_weights)
    c = [-lam[0]] + [lam[l - 1] - lam[l] for l in range(1, N_TIERS)] + [lam[-1]]
    return torch.tensor(c, dtype=torch.float32)


# --------------------------------------------------------------------------- heads
class MultitaskHead(torch.nn.Module):
    """One Linear per taxonomy tier on shared features (hierarchy.py:19-47)."""

    def __init__(self, num_features, num_classes):
        super().__init__()
        self.num_classes = tuple(num_classes)
        for n in self.num_classes:
            assert n > 0
        self.heads = torch.nn.ModuleList([torch.nn.Linear(num_features, n) for n in self.num_classes])

    def forward(self, x):
        from .options import OPTIONS
        ws = [h.weight for h in self.heads]
        if OPTIONS.head_gemm and torch.is_autocast_enabled() and ops.head_supported(x, ws):
            # all tiers as one GEMM over the concatenated classes (libhvk head kernels)
            return list(ops.head_linear(x, ws, [h.bias for h in self.heads]))
        return [head(x) for head in self.heads]


def multitask_surgery(model, head: str, num_classes):
    """Replace `model.<head>` with a MultitaskHead (hierarchy.py:50-62)."""
    if not hasattr(model, head):
        raise RuntimeError(f"model has no attribute {head}!")
    num_features = max(getattr(model, head).weight.shape)
    setattr(model, head, MultitaskHead(num_features, num_classes))


# --------------------------------------------------------------------------- losses
class MultitaskCrossEntropy(torch.nn.Module):
    """sum_l coeffs[l] * CE(inputs[l], targets[l]) (hierarchy.py:65-94), all tiers in
    one kernel launch.  targets: LongTensor [B, tiers], or a list of per-tier
    probability targets (LabelSmoothing)."""

    def __init__(self, *args, coeffs=(1.0,), **kwargs):
        super().__init__()
        if isinstance(coeffs, torch.Tensor):
            coeffs = coeffs.clone().detach().float()
        else:
            coeffs = torch.tensor(list(coeffs), dtype=torch.float)
        self.register_buffer("coeffs", coeffs)
        self._off = {}

    def _offsets(self, sizes, device):
        key = (tuple(sizes), str(device))
        if key not in self._off:
            self._off[key] = torch.tensor(np.r_[0, np.cumsum(sizes)], dtype=torch.int32, device=device)
        return self._off[key]

    def forward(self, inputs, targets):
        assert len(inputs) == len(self.coeffs), f"{len(inputs)} != {len(self.coeffs)}"
        sizes = [z.shape[1] for z in inputs]
        logits = torch.cat([z.float() for z in inputs], dim=1)
        off = self._offsets(sizes, logits.device)
        if isinstance(targets, list):
            assert len(targets) == len(inputs), f"{len(targets)} != {len(inputs)}"
            soft = torch.cat([t.float() for t in targets], dim=1)
            return ops.multitask_cross_entropy(logits, off, self.coeffs, soft=soft)
        assert targets.shape[1] == len(inputs)
        return ops.multitask_cross_entropy(logits, off, self.coeffs, targets=targets)


def soft_cross_entropy(input, target):
    """Flat CE for int or probability targets (composer.loss.soft_cross_entropy as
    called at models.py:112) -- one-head case of the multitask kernel."""
    off = torch.tensor([0, input.shape[1]], dtype=torch.int32, device=input.device)
    one = torch.ones(1, device=input.device)
    if target.dtype.is_floating_point:
        return ops.multitask_cross_entropy(input.float(), off, one, soft=target)
    return ops.multitask_cross_entropy(input.float(), off, one, targets=target.reshape(-1, 1))


class HierarchicalCrossEntropy(torch.nn.Module):
    """HXE (Bertinetto et al., CVPR 2020) over leaf logits.  The reference only
    stubs it (hierarchy.py:183-185) and exposes the knobs hxe_tree_weights /
    hxe_alpha (configs.py:93-96): parity unpinned, pinned by closed-form tests.

    forward(logits [B, n_leaves], targets [B, 7] tier ids or [B] leaf ids), or floating-point
    targets [B, n_leaves]: non-negative leaf weights t (LabelSmoothing's smoothed leaf column),
    the loss then being the expectation sum_c t_c L(c) of the hard loss."""

    def __init__(self, taxonomy: Taxonomy, tree_weights="uniform", alpha=0.1):
        super().__init__()
        self.taxonomy = taxonomy
        self.register_buffer("level_coeff", hxe_level_coeffs(tree_weights, alpha))

    def forward(self, logits, targets):
        if isinstance(targets, list):
            raise NotImplementedError("HXE takes one target tensor over the leaves, not a "
                                      "per-tier list (that is the multitask loss's form)")
        if targets.dtype.is_floating_point:
            if targets.shape != logits.shape:
                raise ValueError(f"soft HXE targets {tuple(targets.shape)} != logits "
                                 f"{tuple(logits.shape)}")
            perm, rank_off, lo, hi, anc = self.taxonomy.device_soft_tables(logits.device)
            return ops.hierarchical_cross_entropy_soft(logits, targets, perm, rank_off, lo, hi,
                                                       anc, self.level_coeff)
        perm, start, end, base, paths = self.taxonomy.device_tables(logits.device)
        if targets.ndim == 1:
            targets = paths[targets]
        return ops.hierarchical_cross_entropy(logits, targets, perm, start, end, base,
                                              self.level_coeff)


class SoftLabelsCrossEntropy(torch.nn.Module):
    """The soft-labels loss of Bertinetto et al. (CVPR 2020, section 3.2) over leaf logits: the
    cross-entropy against t^(c)_k = w_{d(c,k)} / Z_c, w_l = exp(-beta l / 7), d the tree distance
    (build_tree_dist_matrix's entry) and Z_c the sum over k.  The reference has no such loss:
    parity unpinned, pinned by a float64 restatement and closed-form tests.

    forward(logits [B, n_leaves], targets [B, 7] tier ids or [B] leaf ids), or floating-point
    targets [B, n_leaves]: non-negative leaf weights q (LabelSmoothing's smoothed leaf column),
    the loss then being the expectation sum_c q_c L(c) of the hard loss.  `level_weights`: 8
    weights w_0 .. w_7 in place of beta's."""

    def __init__(self, taxonomy: Taxonomy, beta=15.0, level_weights=None):
        super().__init__()
        self.taxonomy = taxonomy
        self.beta = float(beta)
        w = soft_label_level_weights(beta) if level_weights is None \
            else torch.as_tensor(level_weights, dtype=torch.float32).reshape(-1).cpu()
        self._weights = tuple(w.tolist())  # the host copy: the key of Taxonomy.soft_label_norms
        taxonomy.soft_label_norms(self._weights)  # validates
        self.register_buffer("level_weight", w)

    def forward(self, logits, targets):
        if isinstance(targets, list):
            raise NotImplementedError("the soft-labels loss takes one target tensor over the "
                                      "leaves, not a per-tier list (that is the multitask "
                                      "loss's form)")
        if targets.dtype.is_floating_point:
            if targets.shape != logits.shape:
                raise ValueError(f"dense soft-labels targets {tuple(targets.shape)} != logits "
                                 f"{tuple(logits.shape)}")
            perm, rank_off, lo, hi, anc = self.taxonomy.device_soft_tables(logits.device)
            inv_norm = self.taxonomy.soft_label_norms(self._weights, logits.device)
            return ops.soft_labels_cross_entropy_dense(logits, targets, inv_norm, perm, rank_off,
                                                       lo, hi, anc, self.level_weight)
        perm, start, end, base, paths = self.taxonomy.device_tables(logits.device)
        if targets.ndim == 1:
            targets = paths[targets]
        return ops.soft_labels_cross_entropy(logits, targets, perm, start, end, base,
                                             self.level_weight)


class ConditionalSoftmaxCrossEntropy(torch.nn.Module):
    """The conditional (hierarchical) softmax over the MultitaskHead's node logits (Redmon &
    Farhadi, CVPR 2017; Valmadre, NeurIPS 2022): the softmax of a node runs over its siblings only,
    a leaf's probability is the product of the conditionals along its path, and the loss is
    sum_t coeffs[t] * -log p(y_t | y_{t-1}) (ops.cond_softmax_cross_entropy, hvk_cond_softmax_fwd /
    _bwd), the batch mean.  The reference has no such loss: parity unpinned, pinned by a float64
    restatement and closed-form tests.

    forward(outputs: the list of 7 tier logits, targets [B, 7] tier ids or [B] leaf ids).
    `coeffs`: 7 tier coefficients, None or empty = 1 each; `smoothing`: label smoothing WITHIN the
    target's sibling group, in [0, 1).  Per-tier probability targets (LabelSmoothing's list) are
    refused: smoothing every tier on its own is no distribution over paths."""

    def __init__(self, taxonomy: Taxonomy, coeffs=None, smoothing=0.0):
        super().__init__()
        self.taxonomy = taxonomy
        self.coeffs = tuple(float(c) for c in coeffs) if coeffs is not None and len(coeffs) else (1.0,) * N_TIERS
        self.smoothing = float(smoothing)
        if len(self.coeffs) != N_TIERS:
            raise ValueError(f"coeffs: {N_TIERS} tier coefficients, got {len(self.coeffs)}")
        if not 0.0 <= self.smoothing < 1.0:
            raise ValueError(f"smoothing ({smoothing}) outside [0, 1)")
        self.tier_nll = None  # the last batch's per-tier terms, f32 [B, 7]

    def forward(self, outputs, targets):
        if isinstance(targets, (list, tuple)) or targets.dtype.is_floating_point:
            raise ValueError("the conditional-softmax loss takes integer targets ([B, 7] tier ids or [B] leaf "
                             "ids), not probability targets: smooth within the sibling groups with smoothing=")
        if not isinstance(outputs, (list, tuple)) or [o.shape[1] for o in outputs] != list(self.taxonomy.num_classes):
            raise ValueError(f"the conditional softmax takes the {N_TIERS} tier logits of the taxonomy "
                             f"{list(self.taxonomy.num_classes)}")
        dev = outputs[-1].device
        parents, paths = self.taxonomy.device_parent_tables(dev)
        if targets.ndim == 1:
            targets = paths[targets.long()]
        loss, self.tier_nll, _ = ops.cond_softmax_cross_entropy(
            outputs, targets, parents, *self.taxonomy.device_sibling_tables(dev), coeffs=self.coeffs,
            smoothing=self.smoothing, return_tiers=True)
        return loss


# --------------------------------------------------------------------------- metrics
def fine_grained_predictions(output, topk=1, hierarchy_level=-1):
    """Top-k predictions of the finest tier (hierarchy.py:371-388)."""
    if isinstance(output, list):
        output = output[hierarchy_level]
    maxk = min(topk, output.shape[1])
    return output.topk(maxk, dim=1, largest=True, sorted=True)[1]


def crm_predictions(outputs, tree_dists):
    """CRM decoding (Karthik et al., ICLR 2021): the class of least expected tree distance under
    softmax(outputs), int64 [B]; a list of outputs gives its finest tier's logits, as
    fine_grained_predictions takes them.  `tree_dists`: uint8 [L, L] on the logits' device."""
    if isinstance(outputs, (list, tuple)):
        outputs = outputs[-1]
    targets = torch.zeros(outputs.shape[0], device=outputs.device, dtype=torch.int64)
    state = torch.zeros(EvalMetrics.N_STATE, device=outputs.device, dtype=torch.float64)
    return ops.crm_predict(outputs, targets, tree_dists, state)[0].long()


def _joint_decode(outputs, taxonomy, weights, want_scores):
    if not isinstance(outputs, (list, tuple)) or len(outputs) != N_TIERS:
        raise ValueError(f"joint decoding takes the list of {N_TIERS} tier logits")
    if [o.shape[1] for o in outputs] != list(taxonomy.num_classes):
        raise ValueError(f"tier logits {[o.shape[1] for o in outputs]} do not fit the taxonomy "
                         f"{list(taxonomy.num_classes)}")
    dev = outputs[-1].device
    parents, paths = taxonomy.device_parent_tables(dev)
    targets = torch.zeros(outputs[-1].shape[0], device=dev, dtype=torch.int64)
    state = torch.zeros(EvalMetrics.N_STATE, device=dev, dtype=torch.float64)
    return ops.joint_decode(outputs, targets, parents, paths, weights, state, want_scores=want_scores)


def joint_scores(outputs, taxonomy, weights=None):
    """Joint path decoding of the 7 tier logits (ops.joint_decode, hvk_joint_decode): (scores f32
    [B, L], lse f32 [B]) with log p(k) = scores[:, k] - lse = sum_t w_t log softmax(z_t)[anc_t(k)]
    - log Z, the product of the heads' softmaxes along leaf k's path; weights None = 1 per tier."""
    out = _joint_decode(outputs, taxonomy, weights, True)
    return out["scores"], out["lse"]


def joint_predictions(outputs, taxonomy, weights=None):
    """argmax_k of joint_scores, int64 [B] (the lowest k among equal scores), without storing the
    scores."""
    return _joint_decode(outputs, taxonomy, weights, False)["pred"].long()


def _cond_decode(outputs, targets, taxonomy, state, topk=5, want_scores=False, scores_out=None):
    if not isinstance(outputs, (list, tuple)) or len(outputs) != N_TIERS:
        raise ValueError(f"conditional-softmax decoding takes the list of {N_TIERS} tier logits")
    if [o.shape[1] for o in outputs] != list(taxonomy.num_classes):
        raise ValueError(f"tier logits {[o.shape[1] for o in outputs]} do not fit the taxonomy "
                         f"{list(taxonomy.num_classes)}")
    dev = outputs[-1].device
    parents, paths = taxonomy.device_parent_tables(dev)
    if targets is None:
        targets = torch.zeros(outputs[-1].shape[0], device=dev, dtype=torch.int64)
    if state is None:
        state = torch.zeros(EvalMetrics.N_STATE, device=dev, dtype=torch.float64)
    return ops.cond_softmax_decode(outputs, targets, parents, *taxonomy.device_sibling_tables(dev), paths, state,
                                   topk=topk, want_scores=want_scores, scores_out=scores_out)


def cond_softmax_scores(outputs, taxonomy):
    """The leaf log-probabilities f32 [B, L] of the conditional softmax over the 7 tier logits
    (ops.cond_softmax_decode, hvk_cond_softmax_decode): log p(k) = sum_t log p(anc_t(k) | anc_{t-1}(k)),
    normalised by construction.  They are [B, L] scores like any leaf logits: crm_predictions,
    backoff_predictions and BackoffMetrics take them as they are."""
    return _cond_decode(outputs, None, taxonomy, None, want_scores=True)["scores"]


def cond_softmax_predictions(outputs, taxonomy):
    """argmax_k of cond_softmax_scores, int64 [B] (the lowest k among equal scores), without
    storing the scores."""
    return _cond_decode(outputs, None, taxonomy, None)["pred"].long()


def _backoff_decode(outputs, targets, taxonomy, thresholds, state):
    if isinstance(outputs, (list, tuple)):
        outputs = outputs[-1]
    if outputs.ndim != 2 or outputs.shape[1] != taxonomy.num_leaves:
        raise ValueError(f"logits {tuple(outputs.shape)} do not fit the taxonomy's {taxonomy.num_leaves} leaves")
    dev = outputs.device
    return ops.backoff_decode(outputs, targets, *taxonomy.device_backoff_tables(dev),
                              taxonomy.device_parent_tables(dev)[1], thresholds, state)


def backoff_predictions(outputs, taxonomy, threshold=0.5):
    """Back-off decoding (Deng et al., CVPR 2012; ops.backoff_decode, hvk_backoff_decode): descend
    the taxonomy from the root, at every node to the child of largest mass (the softmax summed over
    the child's leaves; the lowest node_start among equal masses), and stop at the last depth whose
    mass is at least `threshold` (in (0, 1]).  Returns {"path": int64 [B, 7], the tier ids of the
    greedy path and the leaf id last; "prob": f32 [B, 7], the masses along it, descending; "depth":
    int64 [B], the entries of the path that stand: 0 answers with the root alone, 7 with a leaf}.
    The path itself does not depend on the threshold, and its leaf need NOT be the argmax leaf: a
    leaf may lead its row and still sit in a genus lighter than its neighbour.

    A list of outputs gives its finest tier's logits, as crm_predictions takes them; any [B, L]
    scores whose softmax is the distribution meant may be passed, so joint_scores(...)[0] backs a
    multitask checkpoint off on its joint distribution."""
    th = ops.backoff_thresholds((threshold,))
    last = outputs[-1] if isinstance(outputs, (list, tuple)) else outputs
    targets = torch.zeros(last.shape[0], device=last.device, dtype=torch.int64)
    state = torch.zeros(BackoffMetrics.N_FIXED + BackoffMetrics.N_SUMS, device=last.device, dtype=torch.float64)
    out = _backoff_decode(outputs, targets, taxonomy, th, state)
    tau = torch.tensor(th[0], dtype=torch.float32, device=last.device)  # the kernel's own comparison
    return {"path": out["path"].long(), "prob": out["prob"], "depth": (out["prob"] >= tau).sum(1)}


class BackoffMetrics(torch.nn.Module):
    """The operating points of back-off decoding (backoff_predictions' rule) at every threshold of
    `thresholds` (ascending, each in (0, 1], at most 32), from one kernel pass per batch
    (ops.backoff_decode): the hierarchical precision / recall curve of Valmadre (NeurIPS 2022), at
    leaf depth the risk-coverage curve of selective classification.  With D the stopping depth of a
    row, m the leading depths on which the greedy path agrees with the target's and N the rows,
    compute() returns per threshold tau (keyed f"...@{tau:g}"):
      backoff/depth@tau          sum D / N
      backoff/acc@tau            rows with D <= m / N (the answer is the target or an ancestor)
      backoff/hP@tau             sum min(D, m) / sum D
      backoff/hR@tau             sum min(D, m) / 7 N
      backoff/leaf-coverage@tau  rows with D = 7 / N
      backoff/leaf-acc@tau       rows with D = 7 and m = 7 / rows with D = 7
    (NaN where a denominator is empty).  update(outputs, targets) takes what EvalMetrics.update
    takes: logits or a list whose finest tier counts, leaf ids or [B, T] labels whose last column
    counts.  The running sums are `state`, 2 + 5 T doubles on the device (include/hvk.h), the
    module's only state_dict entry; update() launches without a host synchronisation, compute() is
    the one device-to-host read and sums over the ranks when torch.distributed is initialised."""

    N_FIXED, N_SUMS = 2, 5

    def __init__(self, taxonomy, thresholds=(0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)):
        super().__init__()
        if taxonomy is None:
            raise ValueError("BackoffMetrics needs a taxonomy")
        self.thresholds = ops.backoff_thresholds(thresholds)
        self.taxonomy = taxonomy
        self.register_buffer("state", torch.zeros(self.N_FIXED + self.N_SUMS * len(self.thresholds),
                                                  dtype=torch.float64))
        self.path = self.prob = self.match = None  # the last batch's rows

    def reset(self):
        self.state.zero_()

    @torch.no_grad()
    def update(self, outputs, targets):
        last = outputs[-1] if isinstance(outputs, (list, tuple)) else outputs
        if targets.dtype.is_floating_point:
            raise ValueError("BackoffMetrics takes integer class targets")
        if self.state.device != last.device:
            self.to(last.device)
        out = _backoff_decode(outputs, targets, self.taxonomy, self.thresholds, self.state)
        self.path, self.prob, self.match = out["path"], out["prob"], out["match"]

    def compute(self):
        state = self.state
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            state = state.clone()
            torch.distributed.all_reduce(state, op=torch.distributed.ReduceOp.SUM)
        s = state.tolist()  # the one device-to-host read
        if s[1] != 0:
            raise ValueError(f"{int(s[1])} target(s) outside [0, num_classes) were passed to update()")
        n = s[0]
        div = lambda x, d: x / d if d else float("nan")  # noqa: E731
        out = {}
        for j, tau in enumerate(self.thresholds):
            depth, correct, common, at_leaf, leaf_hit = s[self.N_FIXED + self.N_SUMS * j:][:self.N_SUMS]
            out[f"backoff/depth@{tau:g}"] = div(depth, n)
            out[f"backoff/acc@{tau:g}"] = div(correct, n)
            out[f"backoff/hP@{tau:g}"] = div(common, depth)
            out[f"backoff/hR@{tau:g}"] = div(common, N_TIERS * n)
            out[f"backoff/leaf-coverage@{tau:g}"] = div(at_leaf, n)
            out[f"backoff/leaf-acc@{tau:g}"] = div(leaf_hit, at_leaf)
        return out


class _SumMetric(torch.nn.Module):
    """Minimal torchmetrics-style accumulator (update / compute / reset)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("num", torch.zeros((), dtype=torch.float64))
        self.register_buffer("den", torch.zeros((), dtype=torch.float64))

    def reset(self):
        self.num.zero_()
        self.den.zero_()

    def compute(self):
        return (self.num / self.den).float()


class FineGrainedAccuracy(_SumMetric):
    """Top-k accuracy of the finest tier (hierarchy.py:97-123)."""

    def __init__(self, topk=1):
        super().__init__()
        self.topk = topk

    def update(self, outputs, targets):
        assert isinstance(outputs, list) and targets.ndim > 1
        preds = fine_grained_predictions(outputs, topk=self.topk).view(-1, self.topk)
        tgt = targets[:, -1].view(-1, 1).expand(preds.shape)
        self.num += (preds == tgt).sum()
        self.den += tgt.numel() / self.topk


class Accuracy(_SumMetric):
    """torchmetrics.Accuracy(task="multiclass", num_classes, top_k) with its default micro
    average, as models.py:87-97 builds it: a sample counts when its target is among the top_k
    logits.  Hard taxonomy targets [B, tiers] (the HXE variant's) score the leaf column."""

    def __init__(self, num_classes, top_k=1):
        super().__init__()
        if top_k > num_classes:
            raise ValueError(f"top_k ({top_k}) > num_classes ({num_classes})")
        self.num_classes = num_classes
        self.top_k = top_k

    def update(self, preds, targets):
        if targets.dtype.is_floating_point:
            raise ValueError("Accuracy takes integer class targets")
        if targets.ndim == 2:
            targets = targets[:, -1]
        top = preds.topk(self.top_k, dim=1, largest=True, sorted=True)[1]
        self.num += (top == targets.view(-1, 1)).any(dim=1).sum()
        self.den += targets.numel()


class TreeDistance(_SumMetric):
    """Mean tree distance of the top-1 prediction (hierarchy.py:126-154)."""

    def __init__(self, tree_dists):
        super().__init__()
        self.register_buffer("tree_dists", tree_dists)

    def update(self, outputs, targets):
        preds = fine_grained_predictions(outputs, topk=1).squeeze()
        targets = targets.squeeze()
        self.num += self.tree_dists[preds, targets].sum()
        self.den += targets.numel()


class FineGrainedTreeDistance(TreeDistance):
    def update(self, outputs, targets):
        assert isinstance(outputs, list) and targets.ndim > 1
        super().update(outputs[-1], targets[:, -1])


class CrossEntropyMetric(_SumMetric):
    """Running mean cross-entropy (composer.metrics.CrossEntropy semantics)."""

    def update(self, preds, targets):
        if not targets.dtype.is_floating_point and targets.ndim == 2:
            targets = targets[:, -1]  # HXE: [B, tiers] taxonomy targets, the leaf column
        b = preds.shape[0]
        self.num += soft_cross_entropy(preds, targets).detach().double() * b
        self.den += b


class FineGrainedCrossEntropy(CrossEntropyMetric):
    """CE of the finest tier only (hierarchy.py:170-180)."""

    def update(self, preds, targets):
        if not isinstance(preds, list):
            raise RuntimeError("FineGrainedCrossEntropy needs a list of predictions")
        super().update(preds[-1], targets[:, -1])


class EvalMetrics(torch.nn.Module):
    """acc@1, acc@topk, cross-entropy and tree distance (models.py:61-101) from ONE kernel pass
    over the logits (ops.eval_metrics, hvk_eval_metrics): the fused counterpart of the metric
    classes above, which each re-derive their answer from the logits on their own.

    `tree_dists` (uint8 or f32 [L, L], build_tree_dist_matrix) or `taxonomy` gives "tree-dist";
    a taxonomy compares the 7-tier paths instead of reading the L * L matrix (the same number)
    and adds the per-tier top-1 accuracies.  Ties follow one rule: equal logits rank by index,
    lowest first (a stable descending sort).

    decoding="crm" also scores the CRM prediction of every row (ops.crm_predict: the class of
    least expected tree distance under the row's softmax) as "acc@1/crm" and "tree-dist/crm",
    into the same state; it needs `tree_dists` as uint8, or a `taxonomy`, whose matrix is then
    built once on the device (ops.tree_dist_matrix).  The default "argmax" launches nothing more.

    decoding="joint" is for multitask checkpoints: besides the pass over the species head it
    combines the 7 heads along every leaf's path (ops.joint_decode, weights `tier_weights`, None =
    1 each) and scores that distribution into a second buffer `joint_state` (the same slots, slot
    15 = rows whose heads' argmaxes form one path): "acc@1/joint", "acc@{topk}/joint",
    "cross-entropy/joint", "tree-dist/joint", "acc@1/joint/tier0".."tier6", "path-consistency".
    "joint-crm" also runs CRM on the joint scores: "acc@1/joint-crm", "tree-dist/joint-crm".  Both
    need a `taxonomy` and list outputs of 7 tiers.

    decoding="cond" is for conditional-softmax checkpoints (ConditionalSoftmaxCrossEntropy): the 7
    tier outputs are node logits, decoded into the leaf distribution log p(k) = sum_t log p(anc_t(k)
    | anc_{t-1}(k)) (ops.cond_softmax_decode), and the standard keys -- "acc@1", "acc@{topk}",
    "cross-entropy", "tree-dist", "acc@1/tier0".."tier6" -- are THAT distribution's, in `state`; the
    species logits alone mean nothing there.  "cond-crm" also runs CRM on the decoded scores:
    "acc@1/crm", "tree-dist/crm".  Both need a `taxonomy` and list outputs of 7 tiers.

    The running sums are `state`, 16 doubles on the device (layout: include/hvk.h); it is the
    module's only state_dict entry (with `joint_state` for the joint decodings).  update() launches and returns without a host
    synchronisation, so it can be captured in a HIP graph (move the module to the device first);
    compute() is the one device-to-host read."""

    N_STATE = 16

    DECODINGS = ("argmax", "crm", "joint", "joint-crm", "cond", "cond-crm")

    def __init__(self, tree_dists=None, taxonomy=None, topk=5, decoding="argmax", tier_weights=None):
        super().__init__()
        if topk < 1:
            raise ValueError(f"topk ({topk}) < 1")
        if decoding not in self.DECODINGS:
            raise ValueError(f"decoding must be one of {self.DECODINGS}, got {decoding!r}")
        if decoding == "crm" and tree_dists is None and taxonomy is None:
            raise ValueError("decoding='crm' needs tree_dists or a taxonomy")
        self.joint = decoding in ("joint", "joint-crm")
        self.cond = decoding in ("cond", "cond-crm")
        if (self.joint or self.cond) and taxonomy is None:
            raise ValueError(f"decoding={decoding!r} needs a taxonomy")
        if tier_weights is not None and (not self.joint or len(tier_weights) != N_TIERS):
            raise ValueError(f"tier_weights: {N_TIERS} weights, with a joint decoding only")
        self.tier_weights = None if tier_weights is None else tuple(float(w) for w in tier_weights)
        self.decoding = decoding
        self._crm_dists = None  # the taxonomy's matrix, built on the first crm update()
        self.topk = int(topk)
        self.taxonomy = taxonomy
        self.register_buffer("state", torch.zeros(self.N_STATE, dtype=torch.float64))
        if self.joint:
            self.register_buffer("joint_state", torch.zeros(self.N_STATE, dtype=torch.float64))
        self.register_buffer("tree_dists", tree_dists, persistent=False)
        paths = None
        if taxonomy is not None:
            paths = torch.from_numpy(np.ascontiguousarray(taxonomy.leaf_paths.astype(np.int32)))
        self.register_buffer("leaf_paths", paths, persistent=False)
        self.pred = self.rank = self.nll = self.dist = self.tier_hit = None  # the last batch's rows
        self.crm_pred = self.crm_risk = self.crm_dist = None
        self.joint_pred = self.joint_rank = self.joint_nll = self.joint_lse = self.joint_dist = None
        self.joint_tier_hit = self.head_pred = self.consistent = None
        self.joint_crm_pred = self.joint_crm_risk = self.joint_crm_dist = None

    @property
    def has_dist(self):
        return self.tree_dists is not None or self.leaf_paths is not None

    def reset(self):
        self.state.zero_()
        if self.joint:
            self.joint_state.zero_()

    def _crm_matrix(self):
        """The uint8 [L, L] matrix CRM reads: the one given, else the taxonomy's, built once."""
        if self.tree_dists is not None:
            return self.tree_dists
        if self._crm_dists is None or self._crm_dists.device != self.leaf_paths.device:
            self._crm_dists = ops.tree_dist_matrix(self.leaf_paths)
        return self._crm_dists

    @torch.no_grad()
    def update(self, outputs, targets):
        tiers = outputs
        if (self.joint or self.cond) and (not isinstance(outputs, (list, tuple)) or len(outputs) != N_TIERS):
            raise ValueError(f"decoding={self.decoding!r} takes the list of {N_TIERS} tier logits")
        if isinstance(outputs, (list, tuple)):
            outputs = outputs[-1]  # the finest tier's logits, as FineGrainedAccuracy scores
        if targets.dtype.is_floating_point:
            raise ValueError("EvalMetrics takes integer class targets")
        if self.state.device != outputs.device:
            self.to(outputs.device)
        if self.cond:
            crm = self.decoding == "cond-crm"
            B, L = outputs.shape
            ws = ops._workspace("cond_softmax", outputs.device, 4 * B * L).view(B, L) if crm else None
            out = _cond_decode(tiers, targets, self.taxonomy, self.state, topk=self.topk, want_scores=crm,
                               scores_out=ws)
            self.pred, self.rank, self.nll, self.dist, self.tier_hit = (out[k] for k in
                                                                        ("pred", "rank", "nll", "dist", "tier_hit"))
            if crm:
                self.crm_pred, self.crm_risk, self.crm_dist = ops.crm_predict(out["scores"], targets,
                                                                              self._crm_matrix(), self.state)
            return
        kw = {}
        if self.leaf_paths is not None:  # path mode (also when a matrix was given as well)
            if targets.ndim == 2 and targets.shape[1] == N_TIERS:
                tp = targets.to(torch.int64).contiguous()
                targets = tp
            else:  # leaf ids: their paths, out-of-range ids (counted invalid by the kernel) clamped
                leaf = targets[:, -1] if targets.ndim == 2 else targets
                tp = self.leaf_paths[leaf.long().clamp(0, self.leaf_paths.shape[0] - 1)].to(torch.int64)
            kw = dict(leaf_paths=self.leaf_paths, target_paths=tp, tier_hit=True)
        elif self.tree_dists is not None:
            kw = dict(tree_dists=self.tree_dists)
        self.pred, self.rank, self.nll, self.dist, self.tier_hit = ops.eval_metrics(
            outputs, targets, self.state, topk=self.topk, **kw)
        if self.decoding == "crm":
            self.crm_pred, self.crm_risk, self.crm_dist = ops.crm_predict(outputs, targets, self._crm_matrix(),
                                                                          self.state)
        if self.joint:
            parents, _ = self.taxonomy.device_parent_tables(outputs.device)
            crm = self.decoding == "joint-crm"
            B, L = outputs.shape
            ws = ops._workspace("joint", outputs.device, 4 * B * L).view(B, L) if crm else None
            out = ops.joint_decode(tiers, targets, parents, self.leaf_paths, self.tier_weights, self.joint_state,
                                   topk=self.topk, want_scores=crm, scores_out=ws)
            self.joint_pred, self.joint_rank, self.joint_nll, self.joint_lse = (out[k] for k in
                                                                               ("pred", "rank", "nll", "lse"))
            self.joint_dist, self.joint_tier_hit, self.head_pred, self.consistent = (
                out[k] for k in ("dist", "tier_hit", "head_pred", "consistent"))
            if crm:
                self.joint_crm_pred, self.joint_crm_risk, self.joint_crm_dist = ops.crm_predict(
                    out["scores"], targets, self._crm_matrix(), self.joint_state)

    def compute(self):
        """{"acc@1", "acc@{topk}", "cross-entropy"[, "tree-dist"][, "acc@1/tier0" .. "tier6"]
        [, "acc@1/crm", "tree-dist/crm"][, the "/joint" keys and "path-consistency"]} as
        Python floats over every update() since reset(), summed over the ranks when
        torch.distributed is initialised."""
        state = torch.cat([self.state, self.joint_state]) if self.joint else self.state
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            state = state.clone()
            torch.distributed.all_reduce(state, op=torch.distributed.ReduceOp.SUM)
        s = state.tolist()  # the one device-to-host read
        s, j = s[:self.N_STATE], s[self.N_STATE:]
        if s[5] != 0:
            raise ValueError(f"{int(s[5])} target(s) outside [0, num_classes) were passed to update()")
        n = s[0]
        div = (lambda x: x / n) if n else (lambda x: float("nan"))
        out = {"acc@1": div(s[1]), f"acc@{self.topk}": div(s[2]), "cross-entropy": div(s[3])}
        if self.has_dist:
            out["tree-dist"] = div(s[4])
        if self.leaf_paths is not None:
            for t in range(N_TIERS):
                out[f"acc@1/tier{t}"] = div(s[6 + t])
        if self.decoding in ("crm", "cond-crm"):
            out["acc@1/crm"] = div(s[13])
            out["tree-dist/crm"] = div(s[14])
        if self.joint:
            out.update({"acc@1/joint": div(j[1]), f"acc@{self.topk}/joint": div(j[2]), "cross-entropy/joint": div(j[3]),
                        "tree-dist/joint": div(j[4]), "path-consistency": div(j[15])})
            for t in range(N_TIERS):
                out[f"acc@1/joint/tier{t}"] = div(j[6 + t])
            if self.decoding == "joint-crm":
                out["acc@1/joint-crm"] = div(j[13])
                out["tree-dist/joint-crm"] = div(j[14])
        return out


class LeafCountLookup:
    """Leaves under every node, for split tooling (hierarchy.py:333-368)."""

    def __init__(self, labels):
        self._lookup = collections.defaultdict(int)
        for label in labels:
            for name, v in zip(("kingdom", "phylum", "cls", "order", "family", "genus", "species"),
                               label.clean_tiers):
                self._lookup[(v, name)] += 1
        self.total = len(labels)

    def closest(self, n):
        if isinstance(n, float):
            assert 0 <= n <= 1, "n must be fractional"
            n = int(self.total * n)
        best, dist = None, float("inf")
        for label, count in self._lookup.items():
            if abs(count - n) < dist:
                best, dist = (*label, count), abs(count - n)
        if best is None:
            raise RuntimeError("no values in lookup!")
        return best


def __getattr__(name):
    """HierarchicalNearestCentroid lives where the reference keeps it (hierarchy.py:488-597); it is
    defined in simpleshot.py and resolved on first use, so neither module imports the other at
    load time."""
    if name == "HierarchicalNearestCentroid":
        from .simpleshot import HierarchicalNearestCentroid
        return HierarchicalNearestCentroid
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
