"""deepbedmap_amd -- MI355X-native (gfx950 HIP) drop-in for the ESRGAN hot path of weiji14/deepbedmap.

Mirrors the hot-path interface of the reference's srgan_train.py; every numeric call goes through
libdbm.so (C ABI: include/dbm.h).  There is no CPU fallback: without the built library and an
MI355X the first model/context creation raises.
"""
from ._lib import DbmError, Context, default_context, build  # noqa: F401
from .srgan import (  # noqa: F401
    Adam, DeepbedmapInputBlock, DeviceArray, DiscriminatorModel, GeneratorModel, ResidualDenseBlock,
    ResInResDenseBlock, Variable, calculate_discriminator_loss, calculate_generator_loss, config, global_config,
    infer_num_residual_blocks, load_npz, load_trained_model, optimizers, psnr, save_npz, serializers, ssim_loss_func, to_device, using_config,
)
from .training import (  # noqa: F401
    METRIC_NAMES, MetricsLog, SerialIterator, TrialPruned, compile_srgan_model, concat_examples, dataset_to_device, device_batch, get_train_dev_iterators,
    save_model_weights_and_architecture, split_dataset_random, train_epochs, train_eval_discriminator, train_eval_generator, train_iteration, train_minibatch, trainer,
)
from .parallel import DataParallel, shard_batch, shard_slice  # noqa: F401
from .evaluation import (DevicePoints, GridGeometry, TrackDescription, TrackStats, describe_errors, error_histogram,  # noqa: F401
                         get_deepbedmap_test_result, grdtrack, make_test_area_score)
from .comparison import compare_on_tracks, cubic_bedmap, describe_on_tracks, rescale, standard_deviation_2d  # noqa: F401
from .gridding import block_geometry, block_shape, blockmedian, blockmedian_grid, get_region, parse_region, region_of, reproject  # noqa: F401
from .gridding import mask_far_from_data, tension_surface, to_pixel_registration, xyz_to_grid  # noqa: F401
from .ascii_table import TextReader, ascii_to_xyz, parse_pipeline, read_text_table  # noqa: F401
from .geotiff import (build_overviews, canvas_to_int16, open_geotiff, overview_pyramid, overview_shapes, read_geotiff,  # noqa: F401
                      read_geotiff_resident, save_array_to_grid, write_geotiff_resident)
from .netcdf import (NetcdfVariable, open_netcdf, read_netcdf, read_netcdf_resident, save_grid_to_netcdf,  # noqa: F401
                     write_netcdf_resident)
from .relief import (ColorTable, adler32_combine, grey_cpt, make_cpt, read_cpt, read_png, relief_image,  # noqa: F401
                     relief_image_host, render_dem, save_png, write_png_resident)
from .perspective import View, grid_minmax, perspective_frame, perspective_image, perspective_image_host, plot_3d_view  # noqa: F401
from .overlay import Layer, draw_layers, draw_layers_host, render_map  # noqa: F401
from .tiling import Raster, fill_gaps, get_deepbedmap_model_inputs, get_window_bounds, selective_tile, tile_training_set  # noqa: F401
from .polygons import (Polygons, mask_outside, polygon_mask, read_polygons, read_tiles_geojson, select_tiles,  # noqa: F401
                       tiles_to_geojson)
from .inference import (Shape, clip_inputs, crop_bounds, group_tiles_by_crop_shape, merge_ranks, predict_tiled,  # noqa: F401
                        predict_tiled_resident, tile_steps)
