"""Self-collision of a robot's sphere model: the readers of the reference's collision files, the arrays of wbcqp_sphere_model, and the numpy
statement of what wbcqp_check_collisions computes on the device (include/wbcqp.h, csrc/wbcqp_collide.hpp).

The reference (src/safety/collision_check.cpp:27-87): every link carries a few spheres, links are grouped into members, and the robot collides
when two spheres of DIFFERENT members are closer than the sum of their radii.  Positions come from `Model.body_placements`.  Host code for tests,
tools and initialisation: the hot path is the HIP kernel.
"""
from __future__ import annotations

import ast
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .model import Model

MAX_SPHERES = 256  # WBCQP_MAX_SPHERES
MAX_MEMBERS = 16   # WBCQP_MAX_MEMBERS

Members = Dict[str, Dict[str, List[List[float]]]]


def _parse_members_yaml(text: str) -> Members:
    """The subset of YAML the reference's collision files use: block mappings by indentation whose leaves are flow sequences of numbers, which may
    continue over several lines (lines are joined while the bracket depth is above zero)."""
    root: dict = {}
    stack: List[Tuple[int, dict]] = [(-1, root)]
    pending_key, pending_indent, pending, depth = None, 0, "", 0
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].rstrip()
        if not line.strip():
            continue
        if depth > 0:  # inside a flow sequence that began on an earlier line
            pending += " " + line.strip()
            depth += line.count("[") - line.count("]")
        else:
            indent = len(line) - len(line.lstrip())
            key, sep, rest = line.strip().partition(":")
            if not sep:
                raise ValueError("collision file: expected 'key:' in %r" % raw)
            while stack[-1][0] >= indent:
                stack.pop()
            rest = rest.strip()
            if not rest:
                child: dict = {}
                stack[-1][1][key.strip()] = child
                stack.append((indent, child))
                continue
            pending_key, pending_indent, pending = key.strip(), indent, rest
            depth = rest.count("[") - rest.count("]") if rest.startswith("[") else 0  # only a value that IS a flow sequence can continue
        if depth == 0:
            stack[-1][1][pending_key] = ast.literal_eval(pending) if pending.startswith("[") else pending
            pending_key = None
    if depth != 0:
        raise ValueError("collision file: a flow sequence is not closed")
    return root


def load_members(path_or_dict: Union[str, os.PathLike, dict]) -> Members:
    """{member: {link: [[x, y, z, d], ...]}} from a file in the reference's schema (etc/talos/collisions/talos_collisions.yaml: a top-level
    `members:` mapping) or from a dict that already holds it (with or without the `members` level).  The links keep the file's order."""
    if isinstance(path_or_dict, dict):
        tree = path_or_dict
    else:
        with open(path_or_dict) as f:
            tree = _parse_members_yaml(f.read())
    members = tree["members"] if "members" in tree else tree
    for mname, links in members.items():
        for link, spheres in links.items():
            for sph in spheres:
                if len(sph) != 4:  # collision_check.cpp:71-72
                    raise ValueError("collisions yaml : sphere data should be an float array of dim 4 (%s / %s)" % (mname, link))
    return members


@dataclass
class SphereTable:
    """The arrays of wbcqp_sphere_model, sorted by member (members sorted by name), file order inside a member."""
    body: np.ndarray      # [n] int32
    member: np.ndarray    # [n] int32, non-decreasing
    centre: np.ndarray    # [n, 3] float64 (numbers read as float32, as the reference reads them)
    diameter: np.ndarray  # [n] float32
    member_names: List[str] = field(default_factory=list)
    skipped: List[str] = field(default_factory=list)  # link names the model does not know: left out, as the reference's loop over model.frames does

    @property
    def n_spheres(self) -> int:
        return int(self.body.size)

    def local_index(self) -> np.ndarray:
        """Place of every sphere inside its member (the i and j of the reference's collision_index())."""
        first = np.searchsorted(self.member, self.member, side="left")
        return (np.arange(self.n_spheres) - first).astype(np.int32)


def resolve_body(model: Model, link: str) -> Optional[int]:
    """The body whose joint frame carries `link`: the parent joint of the model frame of that name; a name X_link the frame table does not hold
    is the link joint X_joint moves (the URDF convention); None when neither exists."""
    if link in model.frame_names:
        return int(model.frame_body[model.frame_names.index(link)])
    if link.endswith("_link") and link[:-5] + "_joint" in model.joint_names:
        return model.joint_names.index(link[:-5] + "_joint")
    return None


def sphere_table(model: Model, members: Union[str, os.PathLike, dict]) -> SphereTable:
    members = load_members(members)
    names = sorted(members)  # std::map order
    if len(names) > MAX_MEMBERS:
        raise ValueError("%d members, at most %d" % (len(names), MAX_MEMBERS))
    body, member, centre, diameter, skipped = [], [], [], [], []
    for k, mname in enumerate(names):
        for link, spheres in members[mname].items():
            b = resolve_body(model, link)
            if b is None:
                skipped.append(link)
                continue
            for sph in spheres:
                s32 = np.asarray(sph, dtype=np.float32)
                body.append(b)
                member.append(k)
                centre.append(s32[:3].astype(np.float64))
                diameter.append(s32[3])
    if len(body) > MAX_SPHERES:
        raise ValueError("%d spheres, at most %d" % (len(body), MAX_SPHERES))
    return SphereTable(body=np.array(body, dtype=np.int32), member=np.array(member, dtype=np.int32),
                       centre=np.array(centre, dtype=np.float64).reshape(-1, 3), diameter=np.array(diameter, dtype=np.float32),
                       member_names=names, skipped=skipped)


def check(model: Model, table: SphereTable, q: np.ndarray) -> Dict[str, np.ndarray]:
    """dict(colliding [B] int32, first_pair [B, 2] int32, n_pairs [B] int32, clearance [B], centres [B, n, 3]) for the states q [B, nq]: the
    five outputs of wbcqp_check_collisions."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    B, n = q.shape[0], table.n_spheres
    half = table.diameter * np.float32(0.5)
    thr = (half[None, :] + half[:, None]).astype(np.float64)  # one float32 addition per pair, then widened
    mem = table.member.astype(np.int64)
    loc = table.local_index().astype(np.int64)
    cross = mem[:, None] < mem[None, :]  # (i, j): every unordered cross-member pair once, i in the member of the smaller number
    key = (mem[:, None] << 20) | (mem[None, :] << 16) | (loc[:, None] << 8) | loc[None, :]  # the order the reference's four loops meet pairs in
    out = {"colliding": np.zeros(B, np.int32), "first_pair": np.full((B, 2), -1, np.int32), "n_pairs": np.zeros(B, np.int32),
           "clearance": np.full(B, np.inf), "centres": np.zeros((B, n, 3))}
    for k in range(B):
        R, p = model.body_placements(q[k])
        c = np.einsum("sij,sj->si", R[table.body], table.centre) + p[table.body]
        out["centres"][k] = c
        d = c[None, :, :] - c[:, None, :]
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        hit = cross & (dist < thr)
        if cross.any():
            out["clearance"][k] = (dist - thr)[cross].min()
        out["n_pairs"][k] = int(hit.sum())
        if hit.any():
            out["colliding"][k] = 1
            flat = int(np.where(hit, key, np.iinfo(np.int64).max).argmin())
            out["first_pair"][k] = divmod(flat, n)
    return out


def pair_names(table: SphereTable, first_pair: Sequence[int]) -> Optional[Tuple[Tuple[str, int], Tuple[str, int]]]:
    """((member, i), (member, j)) of a first_pair row, the reference's collision_index(); None for -1 -1."""
    a, b = int(first_pair[0]), int(first_pair[1])
    if a < 0 or b < 0:
        return None
    loc = table.local_index()
    return ((table.member_names[table.member[a]], int(loc[a])), (table.member_names[table.member[b]], int(loc[b])))
