"""Model hyper-parameters that fix tensor shapes — plain-dict equivalent of experiments/lcrnet/config_model.py:33-93
(same names; no EasyDict, no mkdir side effects)."""


def make_cfg():
    init_voxel = 0.3
    return {
        "seed": 7351,
        "backbone": {"num_stages": 4, "init_voxel_size": init_voxel, "kernel_size": 15, "base_radius": 4.25, "base_sigma": 2.0,
                     "init_radius": 4.25 * init_voxel, "init_sigma": 2.0 * init_voxel, "group_norm": 32, "input_dim": 1,
                     "init_dim": 64, "output_dim": 256},
        "GAT": {"input_dim": 1024, "hidden_dim": 128, "output_dim": 256, "num_heads": 4, "num_layers": 4, "k": None},
        "model": {"num_points_in_patch": 128, "num_sinkhorn_iterations": 100, "ground_truth_matching_radius": 0.45,
                  "ground_truth_corres_radius": 2.4},
        "Vote": {"MAX_TRANSLATE_RANGE": 4.2, "MLPS": [512, 256], "NMS_radius": 2.4},
        "coarse_matching": {"num_targets": 128, "overlap_threshold": 0.1},      # config_model.py:57-58, the training targets
        "fine_matching": {"acceptance_radius": 0.45, "mutual": False, "topk": 1, "confidence_threshold": 0, "use_dustbin": True,
                          "use_global_score": False, "correspondence_threshold": 3, "correspondence_limit": None, "num_refinement_steps": 5},
        "neighbor_limits": [64, 65, 74, 80],     # dataset_loop_detection.py:25,80 (training default)
        # the loss terms (config_model.py:95-122), read by losses.py
        "coarse_loss": {"positive_margin": 0.1, "negative_margin": 1.4, "positive_optimal": 0.1, "negative_optimal": 1.4, "log_scale": 40,
                        "positive_overlap": 0.1},
        "fine_loss": {"positive_radius": 0.45},
        "distribution_loss": {"triplet_loss_gamma": 0.5},
        "triplet_loss": {"margin": 0.5},
        "loss": {"weight_coarse_loss": 1.0, "weight_vote_loss": 0.25, "weight_gap_loss": 5},
        # the Adan optimiser of the loop-detection trainer (config_ld.py:69-79), read by adan.Adan.from_cfg
        "optimadan": {"lr": 1e-4, "lr_decay": 0.95, "lr_decay_steps": 4, "weight_decay": 1e-6, "opt_betas": None, "opt_eps": None,
                      "max_grad_norm": 0, "no_prox": False},
    }
