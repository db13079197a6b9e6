"""`run --exclude_path=<csv>` (ours; no counterpart in the reference): clips the selection must not see.

The first two columns of every line of the file are `shard_name,filename`: the file `clustering/cli.py dedup` writes qualifies
(leave the later copies out), and so does the output.csv of an earlier run ("select more, but not these").  The listed clips are
dropped from (assignments, shard_names, filenames) right after the assignment shards are loaded (run.py: _load, the one place
run_single, the chunk loop and the lockstep groups pass through), so subset.ratio applies to the clips that remain.  A clip is
matched on its shard name and the stem of its file name.  Entries that match no loaded clip are counted and printed, not refused:
a chunk sees only part of the list.  `contrastive` and the pca measures read feature shards, not assignment shards: for them
the key is refused before anything is read.  Without the key every file is what it was."""
import csv
from pathlib import Path

import numpy as np


def check_exclude(measure_name, exclude_path):
    """refused before anything is read: the key with a measure that does not select from assignment shards"""
    if exclude_path is None:
        return
    from .run_pca import is_pca_measure
    name = str(measure_name).lower()
    if name == 'contrastive' or is_pca_measure(name):
        raise ValueError("exclude_path: the measure {!r} reads feature shards, the exclude list applies to the measures that "
                         "select from assignment shards; drop the key or the clips' rows".format(measure_name))


def read_exclude(path):
    """the set of (shard_name, file stem) of a csv whose first two columns are shard_name,filename; empty lines are skipped"""
    keys = set()
    with open(path, newline='') as f:
        for num, row in enumerate(csv.reader(f), 1):
            if not row:
                continue
            if len(row) < 2:
                raise ValueError("{}: line {} has {} column(s), expected shard_name,filename[,...]".format(path, num, len(row)))
            keys.add((row[0], Path(row[1]).stem))
    return keys


def keep_mask(keys, shard_names, filenames):
    """-> (bool [V]: True for the clips that stay, number of entries of `keys` that match no clip)"""
    mine = [(s, Path(f).stem) for s, f in zip(shard_names, filenames)]
    keep = np.array([key not in keys for key in mine], dtype=bool).reshape(len(mine))
    return keep, len(keys - set(mine))


def apply_exclude(keys, loaded):
    """(assignments, clustering_types, shard_names, filenames) without the listed clips, in the order they had; prints the
    count of dropped clips and of entries that matched none"""
    assignments, clustering_types, shard_names, filenames = loaded
    keep, unknown = keep_mask(keys, shard_names, filenames)
    print("exclude_path: dropped {} of {} clips; {} of {} entries match no loaded clip".format(
        int((~keep).sum()), len(keep), unknown, len(keys)))
    ids = np.flatnonzero(keep)
    return (np.ascontiguousarray(np.asarray(assignments)[ids]), clustering_types, [shard_names[i] for i in ids],
            [filenames[i] for i in ids])
