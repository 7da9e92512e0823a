"""rafft_amd - MI355X-native RAFFT folding engine (drop-in for `rafft.fold`).

    from rafft_amd import fold
    structures, trajectory = fold(seq, max_stack=20, traj=True)

The compute path is libraffthip.so (hand-written HIP for gfx950); there is no CPU
fallback - importing works anywhere, calling needs the built library and a GPU."""
from .rafft import fold, fold_batch, submit_batch, eval_structures, eval_structures_info, last_stats  # noqa: F401
from .params import load_params, load_params_from_viennarna, reset_params, save_params, params_info, unpinned_entries  # noqa: F401
from .rafft_kin import kinetics, kinetics_batch  # noqa: F401
from .zuker import mfe, mfe_batch, mfe_span, mfe_span_batch, mfe_span_batch_raw  # noqa: F401
from .zuker import mfe_constrained, mfe_constrained_batch, mfe_constrained_batch_raw, shape_deigan  # noqa: F401
from .cofold import cofold, cofold_batch, cofold_batch_raw, cofold_duplex_init, CofoldResult  # noqa: F401
from .mccaskill import pf, pf_batch, sample, sample_batch  # noqa: F401
from .mccaskill import pf_span, pf_span_batch, pf_span_batch_raw, band_to_dense, band_pairs  # noqa: F401
from .mccaskill import pf_constrained, pf_constrained_batch, pf_constrained_batch_raw  # noqa: F401
from .mccaskill import MeaResult, mea, mea_batch, mea_from_probs, pair_frequencies  # noqa: F401
from .wuchty import subopt, subopt_batch, subopt_batch_raw  # noqa: F401
# (`rafft_amd.findpath` stays the module; its single-problem form is findpath.findpath)
from .findpath import findpath_batch, findpath_batch_raw, path_rows  # noqa: F401
from .descend import descend_batch, descend_batch_raw, minima_batch, basin_graph  # noqa: F401
from .barriers import barriers_batch_raw, barrier_tree, barrier_trees, BarrierTree  # noqa: F401
from .kinfold import kinfold_batch, kinfold_batch_raw, kinfold_weights, first_passage, occupancy  # noqa: F401
# (the function `landscape.landscape` is exported as folding_landscape: `rafft_amd.landscape` stays the module)
from .landscape import landscape as folding_landscape, distance_matrix_gpu, mds_gpu, surface_gpu, Landscape  # noqa: F401
from .utils import Structure, parse_rafft_output, paired_positions, dot_bracket, read_fasta, format_trajectory  # noqa: F401
