from .sgd_clustering import KMeans  # noqa: F401
from .whiten import ColumnMoments, whiten, whiten_  # noqa: F401
from .normalize import normalize, normalize_  # noqa: F401
from .pca import PCA, ScatterMoments, pca_feature, pca_features, project  # noqa: F401
from .lloyd import accumulate, centers_from_sums, fit, fixed_point_shift, lloyd_update, rows_absmax, split_empty  # noqa: F401
from . import kmeanspp  # noqa: F401
from . import silhouette  # noqa: F401
from .silhouette import sample_indices, silhouette_samples, summarise  # noqa: F401
from . import dedup  # noqa: F401
from .dedup import nearest_earlier, nearest_in  # noqa: F401
