"""ABX within / across speakers of quantized units -- cpc/eval/eval_ABX_clustering.py of the reference: same classes
(QuantizedClustering, ClusteringFeatures), same eval_ABX_Librispeech(), same command line, same output JSON.

    python -m cpc2_amd.eval.eval_ABX_clustering --quantized <quantized_outputs.txt> --path_audio_data <dataset dir> \\
        --path_abx_item <file.item> --name-output <scores.json> [--onehot-dict <dict.txt>]
    python -m cpc2_amd.eval.eval_ABX_clustering --clustering <clustering dir>/checkpoint_last.pt --path_audio_data ... \\
        --path_abx_item ... --name-output ... [--soft-clustering] [--group-modes seq|onehot|concat|combine]

What maps to what:

    QuantizedClustering.feature_function    the reference's [1, S, n_units] one-hot tensor, on the GPU
    ClusteringFeatures.feature_function     the reference's soft distances / one-hot / multi-hot tensor; hard assignments come
                                            from kMeanCluster.assign (the fused kernel), never from a [S, k] distance tensor
    *.unit_function (new)                   path -> int64 [S]: the unit id of every frame, where there is exactly one
                                            (`has_units`: --quantized; --clustering with hard assignments and one group, or
                                            the group modes seq / onehot); `n_units` is the width of its one-hot row
    eval_ABX_Librispeech                    the reference's checks, ABX settings (max_x_across=5, max_size_group=10,
                                            normalize=True) and JSON.  With unit_function / n_units it scores the units
                                            through abx_iterators.ABXUnitLoader and cpc_abx_dtw_units: the one-hot matrix is
                                            never built.  Without them (multi-hot concat / combine, soft clustering) it is
                                            eval_ABX.ABX on feature_function, the dense kernels.

Deviations from the reference:

  * --path_audio_data and --path_abx_item are required (the reference defaults to paths of its authors' cluster).
  * --group-modes onehot with more than one group: the reference's feature_function reads a `pair2idx` that only exists as a
    local of __init__ and dies with a NameError; here the dictionary is kept on the object and the mode works.  A frame's token
    joins its n_groups ids (the reference's reshape(-1, 2) is the two-group case of it), as `combine` takes every group's
    stride (the reference's [::2] / [1::2]).
  * --quantized with --group-modes other than onehot is refused (the reference's assert on a tuple never fires).
  * eval_ABX_Librispeech takes three more keyword arguments: unit_function, n_units (the unit path) and seq_list (an
    explicit [(file id, path)] list instead of the unsorted Path.glob, whose order -- and with it the random.sample draws
    -- depends on the file system).
  * --gru and --no-save are parsed and unused, as in the reference (the GRU level comes from the clustering run's
    args.json; the scores are saved when --name-output is given).  The `seq` mode divides --feature-size by
    step_feature_multiplication, as in the reference.
  * A clustering run with --dimReduction is refused (not supported by this package's clustering either).
"""
import argparse
import json
import sys
from os.path import basename, exists, splitext
from pathlib import Path

import torch

from ..clustering.clustering import loadClusterModule
from ..feature_loader import FeatureModule, buildFeature, loadModel
from .ABX import abx_group_computation as abx_g
from .ABX import abx_iterators as abx_it
from .eval_ABX import ABX, score_across, score_within

GROUP_MODES = ["seq", "onehot", "concat", "combine"]


def write_json(filepath, scores):
    Path(filepath).parent.mkdir(parents=True, exist_ok=True)
    with open(filepath, "w") as file:
        json.dump(scores, file, indent=2)


def read_args(pathArgs):
    print(f"Loading args from {pathArgs}")
    with open(pathArgs, "r") as file:
        return argparse.Namespace(**json.load(file))


def read_onehot_dict(path):
    """{token: line index} of a dictionary file, one `token [count]` per line (empty lines keep their index)."""
    print("")
    print(f"Loading onehot dictionary from {path}...")
    with open(path, "r") as f:
        lines = f.read().split("\n")
    return {word.split()[0]: i for i, word in enumerate(lines) if word}


def one_hot(units, n_units):
    """[S] integer units -> [S, n_units] fp32 one-hot rows on the units' device."""
    out = torch.zeros(units.size(0), n_units, dtype=torch.float32, device=units.device)
    out.scatter_(-1, units.long().unsqueeze(1), 1)
    return out


def load_cpc_feature_maker(CPC_path_checkpoint, encoder_layer=False, keepHidden=True, gru_level=-1):
    updateConfig = None
    if gru_level is not None:
        updateConfig = argparse.Namespace(nLevelsGRU=gru_level)
    model = loadModel([CPC_path_checkpoint], updateConfig=updateConfig)[0]
    model.gAR.keepHidden = keepHidden
    feature_maker = FeatureModule(model, encoder_layer)
    feature_maker.eval()
    feature_maker.cuda()
    print("Checkpoint loaded!")
    print("")
    return feature_maker


class ClusteringFeatures:
    def __init__(self, clustering_path_checkpoint, soft_clustering=False, encoder_layer=False, keepHidden=True,
                 group_modes="concat", onehot_dict=None):
        self.group_modes = group_modes
        self.soft_clustering = soft_clustering

        clustering_path_checkpoint = Path(clustering_path_checkpoint)
        assert clustering_path_checkpoint.suffix == ".pt"
        assert self.group_modes in GROUP_MODES
        if (clustering_path_checkpoint.parent / "args.json").is_file():
            path_config = clustering_path_checkpoint.parent / "args.json"
        elif (clustering_path_checkpoint.parent / "checkpoint_args.json").is_file():
            path_config = clustering_path_checkpoint.parent / "checkpoint_args.json"
        else:
            raise RuntimeError(f"Args file not found in the directory {clustering_path_checkpoint.parent}")
        clustering_args = read_args(path_config)
        print("")
        print(f"Clutering args:\n{json.dumps(vars(clustering_args), indent=4, sort_keys=True)}")
        print("-" * 50)
        if getattr(clustering_args, "dimReduction", None) is not None:
            raise SystemExit("the clustering run used --dimReduction, which is not supported")

        level_gru = vars(clustering_args).get("level_gru", None)
        self.featureMaker = load_cpc_feature_maker(clustering_args.pathCheckpoint, encoder_layer=encoder_layer,
                                                   keepHidden=keepHidden, gru_level=level_gru)
        n_features = self.featureMaker.out_feature_dim
        self.clusterModule = loadClusterModule(clustering_path_checkpoint)
        print("Checkpoint loaded!")
        print("")

        self.dim_clusters = self.clusterModule.Ck.shape[-1]
        self.n_clusters = self.clusterModule.Ck.shape[1]
        self.n_groups = n_features // self.dim_clusters
        assert n_features % self.dim_clusters == 0, \
            f"Number of features {n_features} must be divided by the dimension of clusters {self.dim_clusters}"

        self.pair2idx = None
        if self.n_groups > 1 and self.group_modes == "onehot":
            assert onehot_dict is not None, \
                "A dictionary must be given when there are more than one group and in onehot mode!"
            self.pair2idx = read_onehot_dict(onehot_dict)

    def _assign(self, x):
        """[S * n_groups] int64 units of one file: group g of frame s at s * n_groups + g."""
        c_feature = buildFeature(self.featureMaker, x, seqNorm=False, strict=True, maxSizeSeq=64000).cuda()
        c_feature = c_feature.view(1, -1, self.dim_clusters)
        return c_feature, (None if self.soft_clustering else self.clusterModule.assign(c_feature)[0])

    def _tokens(self, q_feature):
        """The dictionary index of every frame's `id-id-...` token."""
        rows = q_feature.detach().cpu().numpy().reshape(-1, self.n_groups)
        idx = [self.pair2idx["-".join(str(i) for i in item)] for item in rows]
        return torch.tensor(idx, dtype=torch.long, device=q_feature.device)

    @property
    def has_units(self):
        """True where every row of feature_function's output is ONE one-hot unit (unit_function is then defined)."""
        return not self.soft_clustering and (self.n_groups == 1 or self.group_modes in ("seq", "onehot"))

    @property
    def n_units(self):
        if self.n_groups > 1 and self.group_modes == "onehot":
            return len(self.pair2idx)
        return self.n_clusters

    def unit_function(self, x):
        """int64 [S'] on the GPU: the unit of every row of feature_function(x) (S' = S * n_groups for `seq`)."""
        if not self.has_units:
            raise ValueError("unit_function: soft clustering and the multi-hot group modes (concat, combine) have no "
                             "single unit per frame; use feature_function")
        q_feature = self._assign(x)[1]
        if self.n_groups > 1 and self.group_modes == "onehot":
            return self._tokens(q_feature)
        return q_feature

    def feature_function(self, x):
        c_feature, q_feature = self._assign(x)
        if self.soft_clustering:
            return self.clusterModule(c_feature)[0]
        if self.n_groups > 1 and self.group_modes == "onehot":
            one_hot_feature = one_hot(self._tokens(q_feature), len(self.pair2idx))
        elif self.n_groups > 1 and self.group_modes == "concat":
            one_hot_feature = one_hot(q_feature, self.n_clusters).view(-1, self.n_clusters * self.n_groups)
        elif self.n_groups > 1 and self.group_modes == "combine":
            one_hot_feature = torch.zeros(q_feature.shape[-1] // self.n_groups, self.n_clusters, dtype=torch.float32,
                                          device=q_feature.device)
            for g in range(self.n_groups):
                one_hot_feature.scatter_(-1, q_feature[g::self.n_groups].unsqueeze(1), 1)
        else:                                          # one group, or `seq`: a row per (frame, group)
            one_hot_feature = one_hot(q_feature, self.n_clusters)
        S, N = one_hot_feature.size()
        return one_hot_feature.view(1, S, N)

    @property
    def step_feature_multiplication(self):
        if self.group_modes == "seq":
            return self.n_groups
        return 1


class QuantizedClustering:
    def __init__(self, quantized_file, onehot_dict=None):
        self.frames_dict = {}
        with open(quantized_file, "r") as f:
            for line in f:
                if line[-1] == "\n":
                    line = line[:-1]
                filename, frames = line.split("\t")
                filename = splitext(basename(filename))[0]
                self.frames_dict[filename] = frames

        frames = next(iter(self.frames_dict.values()))
        if not frames.split(",")[0].isdigit():             # multi-group, eg. 65-241
            assert onehot_dict is not None, \
                "A dictionary must be given when the quantized outputs is not digits (multi-group case)!"

        pair2idx = read_onehot_dict(onehot_dict) if onehot_dict else None

        self.n_units = -1
        for filename in self.frames_dict:
            frames = self.frames_dict[filename].split(",")
            if pair2idx is not None:
                idxs_seq = [pair2idx[item] for item in frames]
            else:
                idxs_seq = [int(item) for item in frames]
            self.n_units = max(self.n_units, max(idxs_seq))
            self.frames_dict[filename] = idxs_seq
        self.n_units += 1                                  # ids start from 0
        print("")
        print(f"Number of quantized units: {self.n_units}")

    has_units = True

    def unit_function(self, x):
        """int64 [S] (host): the unit ids of the file, as read."""
        return torch.tensor(self.frames_dict[splitext(basename(x))[0]], dtype=torch.long)

    def feature_function(self, x):
        one_hot_feature = one_hot(self.unit_function(x), self.n_units)
        N, S = one_hot_feature.size()
        return one_hot_feature.view(1, N, S).cuda()

    @property
    def step_feature_multiplication(self):
        return 1


def ABX_units(unit_function, n_units, path_item_file, seq_list, distance_mode, step_feature, modes, max_x_across=5,
              max_size_group=30, normalize=True):
    """eval_ABX.ABX on unit ids: {'within': score, 'across': score} from an ABXUnitLoader, scored by cpc_abx_dtw_units.
    Same iterators, draws and aggregation as ABX()."""
    ABXDataset = abx_it.ABXUnitLoader(path_item_file, seq_list, unit_function, step_feature, normalize, n_units)
    distance_function = abx_g.get_distance_function_from_name(distance_mode)
    scores = {}

    if 'within' in modes:
        print("Computing ABX within speakers...")
        ABXIterator = ABXDataset.get_iterator('within', max_size_group)
        scores['within'] = score_within(abx_g.get_abx_scores_dtw_on_group(ABXIterator, distance_function,
                                                                          ABXIterator.symmetric))
        print(f"...done. ABX within : {scores['within']}")

    if 'across' in modes:
        print("Computing ABX across speakers...")
        ABXIterator = ABXDataset.get_iterator('across', max_size_group, max_x_across=max_x_across)
        scores['across'] = score_across(abx_g.get_abx_scores_dtw_on_group(ABXIterator, distance_function,
                                                                          ABXIterator.symmetric))
        print(f"...done. ABX across : {scores['across']}")

    return scores


def eval_ABX_Librispeech(path_data, path_item_file, feature_function, modes="within", feature_size=0.01,
                         distance_mode="cosine", file_extension=".flac", debug=False, path_output=None,
                         unit_function=None, n_units=None, seq_list=None):
    save = path_output is not None
    assert modes in ["within", "across", "all"]
    assert distance_mode in ["cosine", "euclidian"]
    if save:
        assert not exists(path_output), f"The output file {path_output} already exists!!"
    if (unit_function is None) != (n_units is None):
        raise ValueError("eval_ABX_Librispeech: unit_function and n_units go together")

    if modes in ["within", "across"]:
        modes = [modes]
    elif modes == "all":
        modes = ["within", "across"]

    step_feature = 1 / feature_size

    if seq_list is None:
        seq_list = list(Path(path_data).glob(f"**/*{file_extension}"))
        if debug:
            seq_list = seq_list[:100]
        seq_list = [(x.stem, str(x)) for x in seq_list]
    elif debug:
        seq_list = list(seq_list)[:100]

    if unit_function is not None:
        scores = ABX_units(unit_function, n_units, path_item_file, seq_list, distance_mode, step_feature, modes,
                           max_x_across=5, max_size_group=10, normalize=True)
    else:
        scores = ABX(feature_function, path_item_file, seq_list, distance_mode, step_feature, modes, cuda=False,
                     max_x_across=5, max_size_group=10, normalize=True)

    if save:
        scores["args"] = {}
        scores["args"]["modes"] = modes
        scores["args"]["feature_size"] = feature_size
        scores["args"]["distance_mode"] = distance_mode
        scores["args"]["path_data"] = str(path_data)
        scores["args"]["file_extension"] = file_extension
        scores["args"]["debug"] = debug
        if debug:
            scores["args"]["debug_size"] = len(seq_list)
        write_json(path_output, scores)

    return scores


def parse_args(argv):
    parser = argparse.ArgumentParser(description="ABX Evaluation on CPC-clustering. Use either --clustering "
                                                 "pathClustering or --quantized pathQuantized")
    group_type_input = parser.add_mutually_exclusive_group(required=True)
    group_type_input.add_argument("--quantized", type=str, default=None,
                                  help="(str) The path of the quantized file of the corresponding eval dataset.")
    group_type_input.add_argument("--clustering", type=str, default=None,
                                  help="(str) The checkpoint of the clustering module.")
    parser.add_argument("--name-output", type=str, default=None,
                        help="(str) The path of the output JSON; nothing is saved without it.")
    parser.add_argument("--modes", choices=["all", "within", "across"], default="all",
                        help="Mode of the ABX evaluation. Default: all.")
    parser.add_argument("--feature-size", type=float, default=0.01, help="1/sample_rate. Default: 0.01 (~100 Hz)")
    parser.add_argument("--gru", type=int, default=-1,
                        help="Unused, as in the reference: the GRU level is the clustering run's level_gru.")
    parser.add_argument("--file-extension", type=str, default=".flac")
    parser.add_argument("--soft-clustering", "-s", action="store_true",
                        help="Whether to use soft clustering (distances to clusters) features.")
    parser.add_argument("--group-modes", choices=GROUP_MODES, default="onehot",
                        help="Method to deal with multiple groups. Default: onehot.")
    parser.add_argument("--onehot-dict", type=str, default=None,
                        help="Path to the dictionary of the quantized units (required when there are more than one group "
                             "and in onehot mode).")
    parser.add_argument("--debug", action="store_true", help="Debug mode: at most 100 files.")
    parser.add_argument("--no-save", action="store_true", help="Unused, as in the reference.")
    parser.add_argument("--path_audio_data", type=str, required=True, help="(str) The path to the audio dataset.")
    parser.add_argument("--path_abx_item", type=str, required=True, help="(str) The path to the ABX .item file.")
    args = parser.parse_args(argv)
    if args.quantized and args.group_modes != "onehot":
        parser.error("only --group-modes onehot is available with --quantized")
    if args.name_output is not None and exists(args.name_output):
        parser.error(f"the output file {args.name_output} already exists")
    return args


def main(argv):
    args = parse_args(argv)

    if args.clustering:
        FeatureMaker = ClusteringFeatures(args.clustering, soft_clustering=args.soft_clustering, encoder_layer=False,
                                          keepHidden=True, group_modes=args.group_modes, onehot_dict=args.onehot_dict)
    else:
        FeatureMaker = QuantizedClustering(args.quantized, onehot_dict=args.onehot_dict)

    print("")
    print(f"Feature function args:\n{json.dumps(vars(args), indent=4, sort_keys=True)}")
    print("-" * 50)

    step_feature_multiplication = FeatureMaker.step_feature_multiplication
    if step_feature_multiplication > 1:
        feature_size = args.feature_size / step_feature_multiplication
    else:
        feature_size = args.feature_size

    units = FeatureMaker.has_units
    return eval_ABX_Librispeech(path_data=args.path_audio_data, path_item_file=args.path_abx_item,
                                feature_function=FeatureMaker.feature_function, modes=args.modes,
                                feature_size=feature_size, distance_mode="cosine", file_extension=args.file_extension,
                                debug=args.debug, path_output=args.name_output,
                                unit_function=FeatureMaker.unit_function if units else None,
                                n_units=FeatureMaker.n_units if units else None)


if __name__ == "__main__":
    main(sys.argv[1:])
