"""The options of the clustering stage that need every row of a view on one rank, and the one rule that refuses them when several
GPUs partition the ROWS (clustering.multi_gpu = striped / reference / rows).  Pure: no device, no file."""


def multi_gpu_mode(args):
    """clustering.multi_gpu: 'views' (default), 'striped', 'reference' or 'rows' -- see config.py"""
    mode = str(args.clustering.multi_gpu or 'views')
    if mode not in ('views', 'striped', 'reference', 'rows'):
        raise ValueError("clustering.multi_gpu must be 'views', 'striped', 'reference' or 'rows', not {!r}".format(mode))
    return mode


def needs_every_row(args, world_size, option, unmerged):
    """ValueError when `option` runs on several GPUs in a mode that partitions the rows; unmerged: what it would have to merge"""
    mode = multi_gpu_mode(args)
    if int(world_size) > 1 and mode != 'views':
        raise ValueError("{} with clustering.multi_gpu={} on {} GPUs: the rows are partitioned over the ranks and the {} are not "
                         "merged across them; use clustering.multi_gpu=views or one GPU".format(option, mode, world_size, unmerged))


def lloyd_rows(args, world_size):
    """True for the one combination that partitions the rows AND merges across the ranks: clustering.algorithm=lloyd with
    clustering.multi_gpu=rows on several GPUs (integer cluster sums, all-reduced; run_clustering._train_clusters_lloyd)"""
    return int(world_size) > 1 and args.clustering.algorithm == 'lloyd' and multi_gpu_mode(args) == 'rows'


def check_whiten(args, world_size):
    """clustering.whiten needs every row of a view on the rank that takes its moments -- or lloyd + rows, whose ranks exchange
    the per-shard moments and merge them in the one-GPU order"""
    if args.clustering.whiten and not lloyd_rows(args, world_size):
        needs_every_row(args, world_size, "clustering.whiten", "column moments")


def check_normalize(args, world_size):
    """clustering.normalize and clustering.spherical are bools; spherical needs algorithm=lloyd (it renormalises the centres after
    every centre update, and the SGD chain has no such step) and implies normalize.  The normalisation is a function of one row,
    so several GPUs need no exchange: allowed with clustering.multi_gpu=views and with lloyd + rows; the partitioned modes of the
    SGD chain are refused.  -> (normalize, spherical) as the run uses them"""
    flags = []
    for key in ('normalize', 'spherical'):
        v = getattr(args.clustering, key)
        v = False if v is None else v  # (a hand-built args tree without the key)
        if not isinstance(v, bool):
            raise ValueError("clustering.{} must be True or False, not {!r}".format(key, v))
        flags.append(v)
    normalize, spherical = flags
    algo = args.clustering.algorithm or 'sgd'
    if spherical and algo != 'lloyd':
        raise ValueError("clustering.spherical=True with clustering.algorithm={}: spherical k-means renormalises the centres to unit "
                         "length after every centre update of batch (Lloyd) k-means; the SGD chain has no such step (its centres "
                         "are running means).  Use clustering.algorithm=lloyd, or clustering.normalize=True alone".format(algo))
    normalize = normalize or spherical
    mode = multi_gpu_mode(args)
    if normalize and int(world_size) > 1 and mode != 'views' and not lloyd_rows(args, world_size):
        raise ValueError("clustering.normalize with clustering.algorithm={} and clustering.multi_gpu={} on {} GPUs: the row "
                         "normalisation is a function of one row, so nothing would have to be merged across the ranks, but no test "
                         "covers the combination; use clustering.multi_gpu=views, one GPU, or algorithm=lloyd with "
                         "multi_gpu=rows".format(algo, mode, world_size))
    return normalize, spherical


def check_pca(args, world_size):
    """clustering.pca_dim needs every row of a view on the rank that takes its scatter matrix, and is a positive integer"""
    dim = args.clustering.pca_dim
    if dim is None:
        return
    if isinstance(dim, bool) or not isinstance(dim, int) or dim < 1:
        raise ValueError("clustering.pca_dim must be a positive integer or None, not {!r}".format(dim))
    needs_every_row(args, world_size, "clustering.pca_dim", "scatter matrices")
