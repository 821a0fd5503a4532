"""Data formats either side of the hot path: SemanticKITTI bit-packed voxel files, point
labels, WaffleIron feature pickles, KITTI-360 velodyne scans and match files, instance-label pickles -> the input contract of `PascoNet.step_inference`
(a0) and the training batch with its label targets (`FrameReader.train_batch`; on the device: `data.targets`), and Lightning
checkpoints -> `PascoNet`."""
from .augment import random_transformation
from .semantic_kitti import (build_item, build_train_item, collate, collate_train, pack_bits, read_instance_label_pickle, read_invalid, read_label,
                             read_occluded, read_occupancy, read_point_instance_labels, read_pointcloud,
                             read_waffleiron_features, transform_coords, transform_scene, unpack_bits, FrameReader)
from .kitti360 import Kitti360FrameReader, build_item_kitti360, read_match_file, read_velodyne
from .instances import instance_labels, remap_lut, semantic_grid, write_instance_pickle
from .checkpoint import load_lightning_state_dict, net_from_checkpoint, remap_reference_state_dict

__all__ = ["build_item", "build_train_item", "collate", "collate_train", "random_transformation", "pack_bits", "unpack_bits", "read_instance_label_pickle", "read_invalid",
           "read_label", "read_occluded", "read_occupancy", "read_point_instance_labels", "read_pointcloud",
           "read_waffleiron_features", "transform_coords", "transform_scene", "FrameReader",
           "Kitti360FrameReader", "build_item_kitti360", "read_match_file", "read_velodyne", "instance_labels", "remap_lut",
           "semantic_grid", "write_instance_pickle", "load_lightning_state_dict", "net_from_checkpoint", "remap_reference_state_dict"]
