"""covest_amd -- MI355X (gfx950) implementation of CovEst's likelihood grid-search
hot path behind the reference's own model API, and of the steps either side of it
(k-mer histogram, histogram down-sampling, result record).  See DESIGN.md."""
__version__ = "0.1.0"

from .models import BasicModel, RepeatsModel, models, select_model  # noqa: F401,E402
from .estimator import CoverageEstimator  # noqa: F401,E402
from .grid import DenseGrid, dense_grid_argmin, optimize_grid, initial_grid  # noqa: F401,E402
from .hist_steps import (load_histogram, save_histogram, process_histogram, sample_histogram,  # noqa: F401,E402
                         compute_coverage_apx)
from .report import print_output  # noqa: F401,E402
from .profile import profile_negll, likelihood_interval, coverage_interval  # noqa: F401,E402
from .information import observed_information, observed_information_batch, sandwich_covariance, wald_intervals, genome_size_se  # noqa: F401,E402
from . import bootstrap  # noqa: F401,E402
from .bootstrap import parametric_bootstrap, draw_histograms, draw_thresholds, model_cells  # noqa: F401,E402
from . import batch  # noqa: F401,E402
from .batch import HistogramBatch  # noqa: F401,E402
from . import poisson  # noqa: F401,E402
from .poisson import truncated_poisson, truncated_poisson_many, truncated_poisson_table  # noqa: F401,E402
from . import simulate  # noqa: F401,E402
from .simulate import random_genome, simulate_reads, SimulatedReads  # noqa: F401,E402
from .simulate import (repeat_plan, repeat_genome, repeat_genome_device, RepeatGenome, genome_spectrum,  # noqa: F401,E402
                       spectrum_to_q)
from . import jackknife  # noqa: F401,E402
from .jackknife import leave_group_out_histograms, read_jackknife, summarize_jackknife, jackknife_batch  # noqa: F401,E402
from . import posterior  # noqa: F401,E402
from .posterior import posterior_classes, PosteriorClasses  # noqa: F401,E402
from . import read_errors  # noqa: F401,E402
from .read_errors import abundance_weights, read_error_scores, ReadErrorScores  # noqa: F401,E402
from .read_errors import correct_reads, ReadCorrections  # noqa: F401,E402
from . import influence  # noqa: F401,E402
from .influence import (score_rows, read_influence, summarize_influence, rows_moments, rows_moments_device,  # noqa: F401,E402
                        ReadInfluence)
# (covest_amd.read_bootstrap is the FUNCTION, as covest_amd.read_jackknife is; the module of the same name is reached by
# `from covest_amd.read_bootstrap import ...`)
from .read_bootstrap import (bootstrap_weights, bootstrap_weights_device, bootstrap_histograms,  # noqa: F401,E402
                             summarize_read_bootstrap, read_bootstrap)
from . import dedup  # noqa: F401,E402
from .dedup import dedup_reads, dedup_reads_device, DedupReads  # noqa: F401,E402
from .simulate import genome_counts  # noqa: F401,E402
# (covest_amd.copy_spectrum is the FUNCTION too; the module: `from covest_amd.copy_spectrum import ...`)
from .copy_spectrum import copy_spectrum, CopySpectrum  # noqa: F401,E402
