from .sgd_clustering import KMeans  # noqa: F401
from .whiten import ColumnMoments, whiten, whiten_  # noqa: F401
from .pca import PCA, ScatterMoments, pca_feature, pca_features, project  # noqa: F401
