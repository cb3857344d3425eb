from .readers import load_expression, load_clinical, load_network  # noqa: F401
from .writers import (write_biomarkers, write_consensus, write_lgroups,
                      write_neighbors, write_scores, write_stability,
                      write_vectors)  # noqa: F401
