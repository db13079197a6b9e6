"""CLI argument handling shared by the two stages.

Behavioural contract of the reference (clustering/code/args.py:11-83 + config.py, and
subset_selection/code/args.py:11-89 + config.py): keyword arguments with dotted names override a
nested default dict (`--a.b.c=v`), unknown keys are created, every `path` entry becomes an absolute
pathlib.Path, and missing attributes read as None (munch.DefaultMunch(None)).
"""
import ast
import copy
from pathlib import Path


class Namespace(dict):
    """dict with attribute access; missing keys read as None (DefaultMunch(None) semantics)."""

    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return self.get(key)

    def __setattr__(self, key, value):
        self[key] = value

    def __deepcopy__(self, memo):
        return Namespace({k: copy.deepcopy(v, memo) for k, v in self.items()})


def _wrap(tree):
    return Namespace({k: _wrap(v) if isinstance(v, dict) else v for k, v in tree.items()})


def _resolve_paths(tree):
    for key, val in tree.items():
        if isinstance(val, dict):
            _resolve_paths(val)
        elif val is not None and (key == 'path' or key.endswith('_file') or key.endswith('_dir')):
            tree[key] = Path(val).resolve()
    return tree


def merge(defaults, overrides):
    """defaults (nested dict) <- {'a.b.c': v}; returns a Namespace tree with resolved paths."""
    tree = copy.deepcopy(defaults)
    for dotted, value in overrides.items():
        node = tree
        parts = dotted.split('.')
        for part in parts[:-1]:
            if not isinstance(node.get(part), dict):
                node[part] = {}
            node = node[part]
        node[parts[-1]] = value
    return _wrap(_resolve_paths(tree))


def parse_cli(argv):
    """`<command> --key=value --flag ...` -> (command, kwargs); values go through literal_eval like
    python-fire does (numbers, booleans, None, lists), everything else stays a string."""
    if not argv:
        raise SystemExit("usage: cli.py <command> [--key=value ...]")
    command, kwargs, i = argv[0], {}, 1
    while i < len(argv):
        tok = argv[i]
        if not tok.startswith('--'):
            raise SystemExit(f"unexpected argument {tok!r}")
        if '=' in tok:
            key, raw = tok[2:].split('=', 1)
        elif i + 1 < len(argv) and not argv[i + 1].startswith('--'):
            key, raw = tok[2:], argv[i + 1]
            i += 1
        else:
            key, raw = tok[2:], 'True'
        try:
            val = ast.literal_eval(raw)
        except (ValueError, SyntaxError):
            val = raw
        kwargs[key] = val
        i += 1
    return command, kwargs


# clustering/code/config.py:1-58 (only the keys the hot path reads; the rest is accepted and ignored)
CLUSTERING_DEFAULTS = {
    'models': ['layer_vggish', 'layer_slow_fast'],
    'model_types': {'audio': ['vggish', 'layer_vggish'], 'visual': ['slow_fast', 'layer_slowfast']},
    'data': {
        'path': 'data',
        'batch_size': 32,
        'resident_bytes': None,  # ours: device budget for feature rows; beyond it the shards stream in groups
        # ours: WHICH rows form the training batches (acav100m_amd/parallel/row_plan.py: loader_stream).
        # 'reference' (default): the batches the reference's DataLoader delivers for this computation.num_workers -- with
        #   num_workers > 0 (its default: 40) whole batches round-robin over worker streams, worker w reading shards [w::num_workers]
        #   (data/clustering.py:17-66,212-228); num_workers = 0: one stream over the shards in order.
        # 'single': the single-stream order whatever num_workers says (rounds 1-5 of this build).  ACAV_LOADER_ORDER overrides.
        'loader_order': 'reference',
        # 'wrap' (default): every stream is get_length() samples (mps/distributed.py:444-460), a short one starts over -- and the
        #   in-process loader (num_workers = 0) continues where it stopped in the next epoch -- webdataset.ResizedDataset as the
        #   reference wraps its dataset (data/clustering.py:61-65).  'drop': whole batches of the rows that exist.  ACAV_LOADER_TAIL overrides.
        'loader_tail': 'wrap',
        'meta': {'path': None},
        'output': {'path': 'output', 'shard_ok_ratio': 0.99},
    },
    'computation': {
        'random_seed': 0,
        'device': 'cuda',
        'num_workers': 40,
        'num_gpus': None,
        'dist_backend': 'nccl',
        'dist_init_method': 'tcp://localhost:9999',
    },
    'clustering': {
        'ncentroids': 32,
        'epochs': 2,
        'cached_epoch': None,
        'resume_training': False,
        'load_cache_from_shard_subset': True,
        # ours: what several GPUs do in training (acav100m_amd/parallel/row_plan.py).
        # 'views' (default): the clusterings are dealt out over the GPUs, every GPU trains its share over ALL rows with the
        #   one-GPU batch stream and epoch count: the N-GPU run writes the files of the one-GPU run.
        # 'striped': the same one-GPU batch stream and epoch count (hence the same files) with the ROWS partitioned: every GPU holds
        #   the rows of its own shards (rank::N) and they travel in bulk to the GPU that runs a clustering's chain.
        # 'reference': the reference's own N-GPU run -- every GPU holds the rows of its own shards (rank::N), rank q feeds
        #   int(batch_size / N) rows per step (data/clustering.py:25) of its rotated stream over ALL shards
        #   (mps/distributed.py:433-437), epochs = ceil(epochs / N) (run_clustering.py:146): the global batch stays
        #   batch_size, N * rows / batch_size steps per epoch.
        # 'rows': a LARGE-BATCH operating point, not the reference's run: batch_size rows of every GPU's own shards per step
        #   (global batch N x batch_size), ceil(epochs / N) epochs -- N x N fewer SGD steps than 'reference' (64 x at N = 8).
        # With clustering.algorithm=lloyd, 'rows' means something else and 'striped' / 'reference' are refused (they name SGD batch
        #   streams): the ROWS are partitioned (rank r reads, holds and labels the shards r::N), the int64 cluster sums are
        #   all-reduced once per view and iteration, clustering.epochs stays the number of iterations, and the N-GPU run writes
        #   the one-GPU run's files bit for bit (parallel/lloyd_rows.py).  clustering.whiten and clustering.init=kmeans++ go with
        #   it; clustering.pca_dim does not.
        'multi_gpu': 'views',
        # ours: divide every feature column by its standard deviation over all rows before clustering (scipy.cluster.vq.whiten,
        # which every clusterer of the reference's correspondence_retrieval/code/clustering.py:54-63 runs first; no centring).
        # One stats pass over the rows before the first epoch (streamed data: one extra read of every shard); the cache file keeps
        # the divisors as 'whiten_std', and a cached run (clustering.cached_epoch) uses the cache's, whatever this switch says.
        # Several GPUs: clustering.multi_gpu=views, or rows with algorithm=lloyd.  False (default): every file stays what it is
        # without the switch.
        'whiten': False,
        # ours: project every view onto its pca_dim leading principal components before clustering (after the whitening, if on):
        # sklearn.decomposition.PCA(n_components=pca_dim).fit_transform, the second half of the front-end of the reference's
        # correspondence_retrieval/code/clustering.py:62-78 (pca.py: pca_features); no whiten=True scaling.  One scatter-matrix
        # pass over the rows before the first epoch (streamed data: one extra read of every shard); a view that is not wider than
        # pca_dim is left alone.  The cache file keeps 'pca_mean', 'pca_components', 'pca_explained_variance' and
        # 'pca_total_variance', and a cached run (clustering.cached_epoch) projects with the cache's, refusing a pca_dim that
        # disagrees.  Several GPUs: clustering.multi_gpu=views only.  None (default): every file stays what it is without the key.
        'pca_dim': None,
        # ours: 'sgd' (default: the chain of sgd_clustering.py, every file stays what it is without the key) or 'lloyd': batch
        # k-means, what the clusterers of the reference's correspondence_retrieval/code/clustering.py run (clustering_func_type
        # 'faiss' / 'scipy', args.py:18: full passes that move every centre to the mean of its rows), after the whitening and the
        # projection if they are on.  `epochs` is then the number of Lloyd iterations (one pass over all rows each, two sweeps:
        # assign, accumulate); the initial centres are the rows randperm(N)[:ncentroids] of the seeded generator; a cache file is
        # written after every iteration, and the loop stops early when an iteration changes no label.  The cached state carries
        # 'algorithm': 'lloyd' with initial_rounds = 0 and reinit = (.7, 1.0): a cached run, the assign stage and `evaluate` then
        # label every row with its plainly nearest centre.  resume_training from a cache of the other algorithm is refused.
        # Several GPUs: clustering.multi_gpu=views (every rank runs every row) or rows (the rows partitioned, see multi_gpu above).
        'algorithm': 'sgd',
        # ours (algorithm=lloyd only): how the initial centres are chosen.  'random' (default: the rows randperm(N)[:ncentroids],
        # every file and every generator draw stays what it is without the key) or 'kmeans++': D^2 sampling (scipy's
        # kmeans2(minit='++'), sklearn's default) on a sample of the rows -- the first init_sample entries of the same randperm --
        # gathered on the device during the pass that reads the initial rows today; every pick is one read-once sweep over the
        # sample (clustering/kmeanspp.py, acav_kmeanspp_seed), the result a pure function of the rows and the seed.  What to turn
        # when `evaluate` reports empty or under-used clusters, or `cluster` reports splits.  A resumed run ignores the three
        # keys.  Several GPUs: clustering.multi_gpu=views or rows (every rank computes the same seeds from the same sample).
        'init': 'random',
        # local trials per k-means++ pick: 1 (default, the classical algorithm), 'auto' = min(16, 2 + floor(ln ncentroids))
        # (sklearn's greedy variant: of the trials' rows the one that lowers the potential most is kept) or an integer in [1, 16]
        'init_trials': 1,
        # rows of the k-means++ sample: None (default) = min(N, 256 * ncentroids) (faiss's max_points_per_centroid), or an
        # integer of at least ncentroids; only the sample has to be resident, the rows themselves may stream
        'init_sample': None,
        # ours: divide every row of every view by its L2 norm, after the whitening and the projection if they are on (faiss's
        # normalize_L2, the step in front of the spherical k-means that the reference's correspondence_retrieval/code/
        # clustering.py runs by default): the clusterer then separates directions, not magnitudes -- a clip's row norm follows
        # loudness and motion energy.  One in-place sweep on the device as the rows arrive there (acav_rows_normalize), a pure
        # function of the row; an all-zero row is left as it is and reported, a row with an inf or NaN is an error.  Works with
        # both algorithms (for sgd it is a row function in front of the unchanged chain: the centres are running means inside the
        # unit ball).  The cache file keeps 'normalize': True, and a cached run (clustering.cached_epoch) and `evaluate` follow the
        # cache, whatever this switch says; True against a cache without the key is refused.  Several GPUs: clustering.multi_gpu=
        # views, or rows with algorithm=lloyd.  False (default): every file stays what it is without the switch.
        'normalize': False,
        # ours (algorithm=lloyd only; implies normalize): spherical k-means -- after every centre update the centres are
        # renormalised to unit length with the same kernel (faiss's Kmeans(spherical=True)).  With unit rows and unit centres the
        # Euclidean argmin of the assign sweep is the cosine argmax.  A cluster whose mean is exactly the zero vector counts as
        # empty (the split rule applies).  The cached state carries 'spherical': True beside 'algorithm': 'lloyd';
        # resume_training continues what the cache says and refuses a switch that contradicts it.  `evaluate` then reports
        # mean_cosine = 1 - inertia / 2.  False (default): every file stays what it is without the switch.
        'spherical': False,
    },
    # ours: the keys of the `dedup` verb (clustering/dedup.py) are read with args.get('dedup') and have no entry here:
    #   dedup.threshold    required, a number in (0, 1]: the cosine to an earlier row of its cluster from which a row is flagged
    #                      (no default: the right value depends on the embedding; the run prints the counts over a grid)
    #   dedup.view         "<model_key>/<layer>": the view whose rows are compared; required when the cache holds several
    #   dedup.out_path     required: the csv of the flagged rows, shard_name,filename,partner_shard_name,partner_filename,similarity
    #   dedup.report_path  optional: the summary as json
    #   dedup.against_path       a brace glob of feature .pkl shards: the held-out set.  Switches the mode: every pool row is
    #                            compared with the rows of THAT set (decontamination; new shards against curated ones), the pool
    #                            streams, only the held-out view has to fit the device.  Without it: the in-cluster dedup
    #   dedup.against_meta_path  required with against_path: the metadata directory of the held-out shards
    #   dedup.blocking           only with against_path: none (default; every pair, n m of them) or cluster (a pool row meets
    #                            only the held-out rows that calc_best gives its label)
    #   dedup.groups       True: every pair of a cluster at cosine >= threshold, their connected components, one kept row per
    #                      group; out_path then lists the rows NOT kept: shard_name,filename,kept_shard_name,kept_filename,
    #                      similarity,group_size.  Refused with against_path and with probes > 1.  The next three need it:
    #   dedup.keep         first (default: a group's first row in shard order) or central (the member nearest to its centre)
    #   dedup.max_pairs    the most pairs a run may hold (default 2^27, 16 bytes each on the device and on the host)
    #   dedup.groups_path  optional: every member of every group, group,group_size,kept,shard_name,filename
    #   dedup.confirm_view       "<model_key>/<layer>", another view than dedup.view: a pair of dedup.view counts only if its
    #                            cosine in this view reaches confirm_threshold too (a re-upload matches in both views, a shared
    #                            slide or song in one).  Needs groups=True, refused with against_path.  Goes with:
    #   dedup.confirm_threshold  a number in (0, 1]: the cosine a pair must reach in confirm_view
    'debug': False,
}

# subset_selection/code/config.py:1-53
SUBSET_DEFAULTS = {
    'data': {'path': 'data', 'output': {'path': 'output.csv'}, 'meta': {'path': None}},
    'computation': {
        'random_seed': 0,
        'num_workers': 40,
        'use_gpu': True,
        'num_gpus': None,
        'dist_backend': 'nccl',
        'dist_init_method': 'tcp://localhost:9967',
        'use_distributed': True,  # contrastive: one worker per GPU, gradients averaged (run_contrastive.py:56-60,118-168)
        'load_async': False,
        # ours: > 1 selects from that many chunks in lockstep on one GPU: batch_mi (own RNG stream each) and every exact-greedy /
        # pair-counting measure (same picks as 1: they draw nothing); not contrastive, not with celf_ratio (run.lockstep_supported).
        # Exact measures, measured per pick and chunk ("Exact greedy"): 10 000-clip chunks 7.8 us alone, 4.2 / 2.4 /
        # 1.7 / 1.3 us at width 2 / 4 / 8 / 16; 100 000-clip chunks 14.5 us alone, 10.5 / 10.9 / 13.3 / 14.1 us: there the device
        # is full from width 4 on and a larger width buys nothing.
        'concurrent_chunks': 1,
    },
    'subset': {'ratio': 0.2, 'size': None},
    # weight_type: None, or linear|log|exp[_<coeff>] / onehot_<layer>: per-layer weights of the clustering pairs
    #   (correspondence_retrieval cluster_pairing.py / pair_weights.py) for the mi, mem_mi and batch_mi measures
    'clustering': {'pairing': 'combination', 'weight_type': None},
    # batch_mi: batch_size candidates are scored per iteration, the best selection_size of them selected.  Supported:
    #   1 <= selection_size <= batch_size <= 1024 and batch_size x clustering pairs <= 8192 (both are clamped to the number of
    #   clips first).  The defaults are the reference CLI's; its paper grids run at batch_size 100 / selection_size 25 (every
    #   correspondence_retrieval search target) -- 6 x fewer iterations, hence permutations of the candidate list, per subset
    # ours: batch.sampler='permutation' | 'draw' is read with args.batch.get('sampler') and has no entry here (missing reads as
    #   'permutation': the whole candidate list is shuffled every iteration on the reference's generator stream).  'draw'
    #   performs only the first batch_size steps of that shuffle -- every batch keeps its distribution, an iteration costs
    #   O(batch_size) instead of O(candidates), the generator stream (hence the selection) is its own; batch_mi only
    #   (run_greedy.check_sampler), and it works with computation.concurrent_chunks
    'batch': {'batch_size': 20, 'selection_size': 4, 'keep_unselected': True},
    'contrastive': {'num_epochs': 3, 'num_warmup_steps': 1, 'base_lr': 2e-4, 'train_batch_size': 128, 'test_batch_size': 128,
                    'cached_epoch': None, 'train_from_cached': False},
    # the pca measures (pca, pca_ip, pca_cs, pca_l1, pca_l2: run_pca.py): every view is whitened (x / std(x, axis=0)) unless
    #   whiten is False, then projected onto its `dim` leading principal components (None: the smallest view width), as the
    #   front-end of the reference's correspondence_retrieval/code/clustering.py:54-78 does for them
    'pca': {'dim': None, 'whiten': True},
    'measure_name': 'batch_mi',
    # celf_ratio: share of the picks of an exact-greedy measure taken by CELF lazy greedy (correspondence_retrieval args.py:32);
    #   0 = plain greedy.  batch_mi and contrastive refuse a nonzero value
    'celf_ratio': 0,
    'shuffle_candidates': True,
    # ours: exclude_path=<csv> (subset_selection/exclude.py) is read with args.get('exclude_path') and has no entry here: the
    #   clips listed in the file's first two columns (shard_name,filename: a `clustering/cli.py dedup` file, or the output.csv of
    #   an earlier run) are dropped right after the assignment shards are loaded, subset.ratio applies to the rest; refused for
    #   contrastive and the pca measures, which read feature shards
    'chunk_size': None,
    'save_cache_as_csvs': True,
    'log_every': 1000,
    'log_times': 10,
    'verbose': True,
    'debug': False,
}
