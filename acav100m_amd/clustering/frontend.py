"""What happens to a view's rows on their way to the device: divided by a std (clustering.whiten, whiten.py), then projected
(clustering.pca_dim, pca.py), then divided by their own L2 norms (clustering.normalize, normalize.py), or none of it.  FrontEnd is the one statement of it: the cache keys and their dtypes, the width
check against the rows, the bytewise comparison `evaluate` refuses disagreeing epochs with, and the application itself."""
import numpy as np

# the cache keys of a projected view (clustering.pca_dim): fp32 [d], fp32 [p, d], f64 [p], f64
PCA_KEYS = ('pca_mean', 'pca_components', 'pca_explained_variance', 'pca_total_variance')


def as_array(v, kind):
    """a cached value (numpy, or a tensor of a reference-written file) -> C-contiguous numpy array of dtype `kind`"""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, kind)


def pca_of(dt):
    """the projection a cached view's attrs hold -> dict(mean, components, explained_variance, total_variance) or None"""
    if dt is None or dt.get('pca_components') is None:
        return None
    return {key[4:]: dt[key] for key in PCA_KEYS}


class FrontEnd:
    """std: fp32 [d] or None; pca: dict(mean fp32 [d], components fp32 [p, d], explained_variance f64 [p], total_variance f64)
    or None; normalize: bool, the rows are L2-normalised last.  The centres of a view live in the space apply() delivers.
    zero_rows / rows_normalized: what the normalisation met in every apply() so far (all-zero rows are left as they are)."""

    def __init__(self, std=None, pca=None, normalize=False):
        self.normalize = bool(normalize)
        self.zero_rows = self.rows_normalized = 0
        self.std = None if std is None else as_array(std, np.float32)
        self.pca = None if pca is None else {
            'mean': as_array(pca['mean'], np.float32), 'components': as_array(pca['components'], np.float32),
            'explained_variance': as_array(pca['explained_variance'], np.float64), 'total_variance': np.float64(pca['total_variance'])}

    @classmethod
    def from_attrs(cls, dt):
        """of a cached view's attrs (None: a view the cache does not hold -> neither stage)"""
        return cls(None if dt is None else dt.get('whiten_std'), pca_of(dt), bool(dt is not None and dt.get('normalize')))

    def to_attrs(self):
        """-> the cache keys of the stages that are set, in file order.  A stage that is not set adds no key."""
        dt = {} if self.std is None else {'whiten_std': self.std}
        if self.pca is not None:
            dt.update((key, self.pca[key[4:]]) for key in PCA_KEYS)
        if self.normalize:
            dt['normalize'] = True
        return dt

    def then(self, nxt):
        """this front-end followed by a stage it does not hold yet (a fresh run sets the std, takes the scatter matrices of
        the whitened rows, then sets the projection, then the row normalisation)"""
        assert (self.std is None or nxt.std is None) and (self.pca is None or (nxt.std is None and nxt.pca is None)) and (
            not self.normalize or (nxt.std is None and nxt.pca is None and not nxt.normalize)), \
            "every stage of a run's front-end is set once, the std before the projection, the row normalisation last"
        return FrontEnd(nxt.std if self.std is None else self.std, nxt.pca if self.pca is None else self.pca,
                        self.normalize or nxt.normalize)

    def width_out(self, d):
        """columns of what apply() delivers for rows of d columns"""
        return d if self.pca is None else self.pca['components'].shape[0]

    def check_width(self, view, d, where=''):
        """ValueError unless every stage is made for rows of d columns; where: ' in <cache file>' or nothing"""
        if self.std is not None and self.std.shape != (d,):
            raise ValueError("whiten_std of view {}{} has shape {}, the rows have {} columns".format('/'.join(view[1:]), where, self.std.shape, d))
        f = self.pca
        if f is not None and (f['components'].ndim != 2 or f['components'].shape[1] != d or f['mean'].shape != (d,)):
            raise ValueError("pca_components of view {}{} has shape {}, the rows have {} columns".format(
                '/'.join(view[1:]), where, f['components'].shape, d))

    def differs(self, other):
        """the first stage that is not the same in both ('whiten_std', 'the pca projection': their bytes; 'the row normalisation':
        the switch) or None"""
        def arrays(f):
            return (None if f.std is None else [f.std]), (None if f.pca is None else list(f.pca.values()))
        for what, a, b in zip(('whiten_std', 'the pca projection'), arrays(self), arrays(other)):
            if (a is None) != (b is None) or any(
                    np.shape(x) != np.shape(y) or np.asarray(x).tobytes() != np.asarray(y).tobytes() for x, y in zip(a or (), b or ())):
                return what
        if self.normalize != other.normalize:
            return 'the row normalisation'
        return None

    def apply(self, t):
        """t [rows, d] on the device -> divided in place by the std (whiten.whiten_), then projected (pca.project: the whitened
        copy is dropped, what comes back is [rows, p]), then divided in place by the row norms (normalize.normalize_)"""
        if self.std is not None and t.shape[0] and t.shape[1]:
            from .whiten import whiten_
            whiten_(t, self.std)
        if self.pca is not None and t.shape[1]:
            from .pca import project
            t = project(t, self.pca['mean'], self.pca['components'])
        if self.normalize and t.shape[0] and t.shape[1]:
            from .normalize import normalize_
            t, zero = normalize_(t if t.is_contiguous() else t.contiguous())
            self.zero_rows += zero
            self.rows_normalized += int(t.shape[0])
        return t
