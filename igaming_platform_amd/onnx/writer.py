"""Minimal ONNX model construction helpers (no ``onnx`` package in the image)."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import schema as S

_NP2ONNX = {np.dtype(np.float32): S.FLOAT, np.dtype(np.int64): S.INT64,
            np.dtype(np.int32): S.INT32, np.dtype(np.float64): S.DOUBLE,
            np.dtype(np.uint8): S.UINT8, np.dtype(np.int8): S.INT8, np.dtype(np.bool_): S.BOOL}
ML_DOMAIN = "ai.onnx.ml"


def tensor(name: str, arr: np.ndarray, raw: bool = True):
    arr = np.ascontiguousarray(arr)
    t = S.TensorProto(name=name, data_type=_NP2ONNX[arr.dtype])
    t.dims.extend(int(d) for d in arr.shape)
    if raw:
        t.raw_data = arr.tobytes()
    elif arr.dtype == np.float32:
        t.float_data.extend(arr.ravel().tolist())
    elif arr.dtype == np.int64:
        t.int64_data.extend(arr.ravel().tolist())
    else:
        t.raw_data = arr.tobytes()
    return t


def attr(name: str, value):
    a = S.AttributeProto(name=name)
    if isinstance(value, float):
        a.type, a.f = S.A_FLOAT, value
    elif isinstance(value, (bool, int, np.integer)):
        a.type, a.i = S.A_INT, int(value)
    elif isinstance(value, S.TensorProto):  # tensor-valued attribute: attr(name, tensor(name, arr))
        a.type = S.A_TENSOR
        a.t.CopyFrom(value)
    elif isinstance(value, (str, bytes)):
        a.type, a.s = S.A_STRING, value.encode() if isinstance(value, str) else value
    elif isinstance(value, np.ndarray) and value.dtype.kind == "f":
        a.type = S.A_FLOATS
        a.floats.extend(value.astype(np.float32).ravel().tolist())
    elif isinstance(value, np.ndarray) and value.dtype.kind in "iu":
        a.type = S.A_INTS
        a.ints.extend(int(v) for v in value.ravel())
    elif isinstance(value, (list, tuple)) and value and isinstance(value[0], (str, bytes)):
        a.type = S.A_STRINGS
        a.strings.extend(v.encode() if isinstance(v, str) else v for v in value)
    elif isinstance(value, (list, tuple)) and value and isinstance(value[0], float):
        a.type = S.A_FLOATS
        a.floats.extend(value)
    elif isinstance(value, (list, tuple)):
        a.type = S.A_INTS
        a.ints.extend(int(v) for v in value)
    else:
        raise TypeError(f"attribute {name}: unsupported value {type(value)}")
    return a


def node(op: str, inputs: Sequence[str], outputs: Sequence[str], name: str = "",
         domain: str = "", **attrs):
    n = S.NodeProto(op_type=op, name=name or f"{op}_{outputs[0]}", domain=domain)
    n.input.extend(inputs)
    n.output.extend(outputs)
    for k, v in attrs.items():
        n.attribute.append(attr(k, v))
    return n


def value_info(name: str, elem_type: int, shape: Sequence):
    v = S.ValueInfoProto(name=name)
    tt = v.type.tensor_type
    tt.elem_type = elem_type
    for d in shape:
        dim = tt.shape.dim.add()
        if isinstance(d, str):
            dim.dim_param = d
        else:
            dim.dim_value = int(d)
    return v


def model(nodes, inputs, outputs, initializers: Iterable = (), name: str = "graph",
          opset: int = 17, ml_opset: int = 3, metadata: Optional[Dict[str, str]] = None):
    g = S.GraphProto(name=name)
    g.node.extend(nodes)
    g.input.extend(inputs)
    g.output.extend(outputs)
    g.initializer.extend(initializers)
    m = S.ModelProto(ir_version=8, producer_name="igaming_platform_amd", producer_version="0.1",
                     graph=g)
    m.opset_import.add(domain="", version=opset)
    if any(n.domain == ML_DOMAIN for n in nodes):
        m.opset_import.add(domain=ML_DOMAIN, version=ml_opset)
    for k, v in (metadata or {}).items():
        m.metadata_props.add(key=k, value=v)
    return m


def save(m, path: str) -> None:
    with open(path, "wb") as f:
        f.write(m.SerializeToString())


def load(path: str):
    with open(path, "rb") as f:
        return S.ModelProto.FromString(f.read())


def tree_attrs(trees: List[Dict[str, np.ndarray]], prefix: str) -> Dict[str, object]:
    """Flatten per-tree arrays into TreeEnsemble attributes.

    Each tree dict: ``feature`` (int, -1 for leaf), ``threshold`` (f32), ``left``/``right``
    (child node ids; true branch = left), ``mode`` (str per node), ``missing_true`` (0/1),
    ``leaf_values`` ([n_nodes, K] for leaves; rows of internal nodes ignored).
    ``prefix`` is ``target`` (regressor) or ``class`` (classifier).
    """
    tids, nids, fids, vals, modes, tn, fn, miss = [], [], [], [], [], [], [], []
    lt, ln, lid, lw = [], [], [], []
    for t, tr in enumerate(trees):
        n = len(tr["feature"])
        for i in range(n):
            leaf = tr["feature"][i] < 0
            tids.append(t)
            nids.append(i)
            fids.append(0 if leaf else int(tr["feature"][i]))
            vals.append(0.0 if leaf else float(tr["threshold"][i]))
            modes.append("LEAF" if leaf else tr["mode"][i])
            tn.append(0 if leaf else int(tr["left"][i]))
            fn.append(0 if leaf else int(tr["right"][i]))
            miss.append(0 if leaf else int(tr["missing_true"][i]))
            if leaf:
                off = int(tr.get("class_offset", 0))
                for k, w in enumerate(np.atleast_1d(tr["leaf_values"][i])):
                    lt.append(t)
                    ln.append(i)
                    lid.append(k + off)
                    lw.append(float(w))
    return {
        "nodes_treeids": np.array(tids, np.int64), "nodes_nodeids": np.array(nids, np.int64),
        "nodes_featureids": np.array(fids, np.int64), "nodes_values": np.array(vals, np.float32),
        "nodes_modes": modes, "nodes_truenodeids": np.array(tn, np.int64),
        "nodes_falsenodeids": np.array(fn, np.int64),
        "nodes_missing_value_tracks_true": np.array(miss, np.int64),
        f"{prefix}_treeids": np.array(lt, np.int64), f"{prefix}_nodeids": np.array(ln, np.int64),
        f"{prefix}_ids": np.array(lid, np.int64), f"{prefix}_weights": np.array(lw, np.float32),
    }


# ai.onnx.ml opset 5 TreeEnsemble integer codes
V5_MODES = {"BRANCH_LEQ": 0, "BRANCH_LT": 1, "BRANCH_GTE": 2, "BRANCH_GT": 3, "BRANCH_EQ": 4, "BRANCH_NEQ": 5,
            "BRANCH_MEMBER": 6}
V5_AGGREGATE = {"AVERAGE": 0, "SUM": 1, "MIN": 2, "MAX": 3}
V5_POST = {"NONE": 0, "SOFTMAX": 1, "LOGISTIC": 2, "SOFTMAX_ZERO": 3, "PROBIT": 4}


def tree_attrs_v5(trees: List[Dict[str, np.ndarray]], trailing_nan: bool = True) -> Dict[str, object]:
    """Flatten per-tree arrays into the attributes of the opset-5 ``TreeEnsemble`` operator.

    The same per-tree dicts as :func:`tree_attrs`, plus ``members``: per node, the member values
    of a ``BRANCH_MEMBER`` node (its ``threshold`` is ignored). Interior nodes and leaves go to
    separate arrays, interior nodes in each tree's own order; a leaf row becomes one
    (target, weight) leaf per non-zero column (column 0 when the row is all zero), so a leaf may
    write one target only: rows with several non-zero columns are rejected. ``class_offset``
    shifts the target id as in :func:`tree_attrs`. A tree that is a single leaf becomes a root
    whose two branches name that leaf."""
    fids, splits, modes, tn, fn, tl, fl, miss, roots = [], [], [], [], [], [], [], [], []
    ltarget, lw, member = [], [], []
    for tr in trees:
        n = len(tr["feature"])
        is_leaf = [tr["feature"][i] < 0 for i in range(n)]
        node_id, leaf_id = {}, {}
        for i in range(n):
            if is_leaf[i]:
                row = np.atleast_1d(np.asarray(tr["leaf_values"][i], np.float32))
                nz = np.flatnonzero(row)
                if len(nz) > 1:
                    raise ValueError("TreeEnsemble (opset 5): a leaf carries one (target, weight) pair")
                k = int(nz[0]) if len(nz) else 0
                leaf_id[i] = len(ltarget)
                ltarget.append(k + int(tr.get("class_offset", 0)))
                lw.append(float(row[k]))
            else:
                node_id[i] = len(fids) + len(node_id)
        if not node_id:  # a single leaf: a root with two leaf branches
            lid = leaf_id[0]
            roots.append(len(fids))
            fids.append(0), splits.append(0.0), modes.append(0), miss.append(0)
            tn.append(lid), fn.append(lid), tl.append(1), fl.append(1)
            continue
        children = {int(c) for i in node_id for c in (tr["left"][i], tr["right"][i])}
        top = [i for i in range(n) if i not in children]
        if len(top) != 1 or is_leaf[top[0]]:
            raise ValueError("tree_attrs_v5: each tree needs exactly one root")
        roots.append(node_id[top[0]])
        for i in range(n):
            if is_leaf[i]:
                continue
            m = tr["mode"][i]
            fids.append(int(tr["feature"][i]))
            modes.append(V5_MODES[m])
            splits.append(0.0 if m == "BRANCH_MEMBER" else float(tr["threshold"][i]))
            miss.append(int(tr["missing_true"][i]))
            for side, ids, flags in ((tr["left"][i], tn, tl), (tr["right"][i], fn, fl)):
                side = int(side)
                ids.append(leaf_id[side] if is_leaf[side] else node_id[side])
                flags.append(int(is_leaf[side]))
            if m == "BRANCH_MEMBER":
                member.append(np.asarray(tr["members"][i], np.float32).ravel())
    a = {
        "nodes_featureids": np.array(fids, np.int64),
        "nodes_splits": tensor("nodes_splits", np.array(splits, np.float32)),
        "nodes_modes": tensor("nodes_modes", np.array(modes, np.uint8)),
        "nodes_truenodeids": np.array(tn, np.int64), "nodes_falsenodeids": np.array(fn, np.int64),
        "nodes_trueleafs": np.array(tl, np.int64), "nodes_falseleafs": np.array(fl, np.int64),
        "nodes_missing_value_tracks_true": np.array(miss, np.int64),
        "tree_roots": np.array(roots, np.int64),
        "leaf_targetids": np.array(ltarget, np.int64),
        "leaf_weights": tensor("leaf_weights", np.array(lw, np.float32)),
    }
    if member:
        nan = np.array([np.nan], np.float32)
        parts = [p for m in member for p in (m, nan)]
        mv = np.concatenate(parts if trailing_nan else parts[:-1])
        a["membership_values"] = tensor("membership_values", mv.astype(np.float32))
    return a
