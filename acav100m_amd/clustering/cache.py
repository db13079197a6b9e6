"""The clustering cache cache_epoch_{e}_{name} (clustering/code/run_clustering.py:55-116): where an epoch's file is, which
file a run loads, reading it, writing it and finding a view in it.  `cluster` (run_clustering.py) and `evaluate` (evaluate.py)
both come through here."""
import pickle
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .. import shards as io
from .frontend import FrontEnd, as_array


def path(args, epoch):
    return Path(args.data.output.path) / "cache_epoch_{}_{}".format(epoch, Path(args.data.path).name)


def locate(args, epoch):
    """the file that is "the cache of epoch e": path() when it exists, else -- under clustering.load_cache_from_shard_subset --
    the cache trained on the largest subset of these shards, else path() (which does not exist)"""
    exact = path(args, epoch)
    if exact.is_file() or not args.clustering.load_cache_from_shard_subset:
        return exact
    want = set(io.brace_expand(Path(args.data.path).name))
    best = None
    for p in Path(args.data.output.path).glob("cache_epoch_{}_*".format(epoch)):
        have = set(io.brace_expand(p.name[p.name.find('shard-'):]))
        if have and not (have - want) and (best is None or len(have) > best[0]):
            best = (len(have), p)
    return exact if best is None else best[1]


def find(saved, view):
    """the attrs of view (kind, model_key, layer) in what read() returned, or None: by the full key, else by (model_key, layer)
    -- a reference-written file does not name the modality.  The file nests {model_key: {layer: attrs}}, so it cannot hold two
    kinds under one (model_key, layer): the second rule has at most one candidate."""
    if view in saved:
        return saved[view]
    return next((val for key, val in saved.items() if key[1:] == view[1:]), None)


def _attrs_of(obj):
    """attrs dict of one cached clustering: ours (a dict), or a pickled KMeans object (the reference's default
    scheme, run_clustering.py:110-116, readable when its class is importable)"""
    if isinstance(obj, dict):
        dt = dict(obj)
    elif hasattr(obj, 'get_attrs'):
        dt = dict(obj.get_attrs())
    else:
        dt = dict(vars(obj))
    for key in ('centers', 'counts'):
        dt[key] = as_array(dt[key], np.float32)
    dt.update(FrontEnd.from_attrs(dt).to_attrs())
    return dt


def read(file):
    """-> {(kind, model_key, layer): attrs} or None.  The file is the reference's nested
    {model_key: {'layer_i' | 'model': KMeans | attrs}} written by torch.save (run_clustering.py:110-116); the flat
    pickle of round 1 is still accepted.  An unreadable file is reported and treated as absent."""
    import torch
    saved = None
    for reader in (lambda f: torch.load(f, map_location='cpu', weights_only=False), pickle.load):
        try:
            with open(file, 'rb') as f:
                saved = reader(f)
            break
        except Exception as exc:  # zip vs pickle stream, missing classes, truncated file ...
            err = exc
    if saved is None:
        print("clustering cache {} is not loadable: {}".format(file, err))
        return None
    try:
        flat = OrderedDict()
        for key, val in saved.items():
            if isinstance(key, tuple):  # round-1 layout: {(kind, model_key, layer): attrs}
                flat[key] = _attrs_of(val)
                continue
            for layer, obj in val.items():
                dt = _attrs_of(obj)
                flat[(dt.pop('_kind', None), key, layer)] = dt
        return flat
    except Exception as exc:
        print("clustering cache {} has an unknown layout: {}".format(file, exc))
        return None


def save(args, epoch, cl, fronts=None):
    """torch.save of {model_key: {layer: attrs}} -- the reference's file and layout (its save_scheme_ver2 form,
    run_clustering.py:110-116: plain attrs instead of pickled objects, so either side can read it).
    fronts: {view: FrontEnd} of a whitened and / or projected run -> the front-end's keys beside '_kind': the centres live in the
    space FrontEnd.apply delivers, and whoever assigns or judges rows with them applies it first.  A view without one adds no key."""
    import torch
    file = path(args, epoch)
    print("saving clustering cache to: {}".format(file))
    file.parent.mkdir(parents=True, exist_ok=True)
    nested = OrderedDict()
    for (kind, mk, layer), km in cl.items():
        dt = km.get_attrs_plain()
        dt['_kind'] = kind
        dt.update((fronts or {}).get((kind, mk, layer), FrontEnd()).to_attrs())
        nested.setdefault(mk, OrderedDict())[layer] = dt
    torch.save(nested, str(file))
