"""Training CLI with the reference's flags (train.py:438-472) on the MI355X path.

    python show-attend-and-tell_amd/train.py --data data/flickr8k --network vgg19 --tf --ado --attention
    python show-attend-and-tell_amd/train.py --synthetic 512 --network resnet152 --tf --ado --attention

Same flags and defaults as the reference (``--perform-test`` is store_true with default True,
so it cannot be disabled, as in train.py:450), plus:
  --synthetic N   N synthetic images (5 captions each is not needed: one caption per row) instead
                  of the Karpathy-JSON dataset;  --vocab for its vocabulary size
  --dtype         bf16 (default, performance) | fp32 (exact parity mode)
  --max-steps     cap batches per epoch (smoke runs)
  --no-overlap    encode each batch just before its decoder step (default: the frozen encoder of
                  batch i+1 runs on a side stream beside batch i's decoder step)
  --encoder-weights  torchvision-layout state_dict of the trunk (weights_only load); without it the
                  trunk is randomly initialised under --seed (no pretrained weights offline).  Either
                  way the trunk actually used is saved as <out>/encoder_<network>.pth and recorded in
                  model_config.json, so generate_caption.py runs the same encoder
  --host-preprocess  resize + normalize on the DataLoader workers (default: workers only decode, the
                  uint8 images travel at native size and sat_images_to_input resamples them on the GPU,
                  bit-identical to PIL's bilinear resize + torchvision's ToTensor / Normalize)
  --workers       decode workers per rank (default 8)
  --beam-eval K   also caption every validation / test batch with batched beam search of width K
                  (Decoder.caption_batch) and log {mode}_beam_bleu1..4 for the generated sentences
                  (default 0 = off: only the reference's teacher-forced argmax BLEU)
  --fine-tune-encoder N  train the last N units of the trunk (resnet152: layer4's identity bottlenecks, N <= 2; vgg19:
                  the block-5 convolutions, N <= 4) with --encoder-lr (default 1e-5) as a second Adam param group;
                  the frozen prefix of batch i+1 still runs ahead on the side stream, the tail runs inside the step;
                  each epoch also saves encoder_<network>_<epoch>.pth, which model_config.json then names
  --cache-features  encode every unique image of each split once before epoch 1, keep the frozen trunk's output per
                  image in HBM (sat_amd.FeatureCache) and train / evaluate from it: the loaders then open no image and
                  a step gathers its rows with one launch.  With --fine-tune-encoder the cached tensor is the
                  activation entering the trainable tail, which still runs inside the step.  Every rank holds the
                  whole cache; a table that would leave less than FeatureCache's reserve of HBM free is refused
  --feature-cache DIR  implies --cache-features; a valid cache file in DIR (same trunk prefix weights, key list,
                  dtype, preprocessing) is loaded instead of filled, and a filled cache is written there (by rank 0)
  --tf-prob P     scheduled sampling (Bengio et al. 2015) while training: at every step a row feeds the ground-truth
                  token with probability P and the model's own argmax of the previous step otherwise (seeded like the
                  dropout masks, a different draw per rank); validation and test follow --tf as before
  --tf-prob-end Q linear decay of that probability from P in epoch 1 to Q in the last epoch (default Q = P); the
                  epoch's value is logged as tf_prob
  --scst          self-critical sequence training (Rennie et al. 2017), the stage after cross-entropy training (--model
                  names the checkpoint to start from): per step a caption is sampled on the device
                  (Decoder.sample), the greedy caption is decoded under no_grad, both are scored on the host and the
                  policy gradient of (sample's reward - greedy's reward) is followed through the token-weighted
                  loss; logs scst_reward_sample, scst_reward_greedy and scst_logp.  Not with --tf / --tf-prob
  --scst-temperature T  temperature of the sampled caption (default 1.0)
  --scst-reward   cider (default: CIDEr-D over token ids, document frequencies from the train split's references) |
                  bleu (sentence BLEU-4 against the image's references) | cider-device (the same CIDEr-D scored on the
                  device by sat_amd.CiderDDevice: the references, their norms and the n-gram table are resident in HBM,
                  the token matrices never leave the device, the advantage is a device subtraction and the step has no
                  device-to-host copy; the logged reward sums live on the device and are read on --log-interval steps)
  --clip-grad-norm C  clip the gradients of every param group (decoder and, with --fine-tune-encoder, the trainable
                  tail) to global L2 norm C inside the Adam step, on the device (sat_amd.Adam(max_grad_norm=C): no host
                  read in the step); a step whose norm is not finite changes nothing and is counted.  Log lines gain
                  grad_norm and skipped_steps (one host read per --log-interval line).  Default: off; C must be > 0
  --bert-embeddings  a local [30522, 768] bert-base-uncased word-embedding table (a tensor, or a
                  state_dict holding embeddings.word_embeddings.weight / embedding.weight)
Multi-GPU: ``python -m torch.distributed.run --nproc-per-node N show-attend-and-tell_amd/train.py ...``
(RCCL data parallel; the batch size is per GPU).  W&B logging is not part of this build; the
reference's scalar names are printed / written as JSON lines instead.
"""
import argparse
import contextlib
import json
import os
import random
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sat_amd  # noqa: E402
else:
    import sat_amd  # noqa: E402
from sat_amd import bleu as bleu_mod  # noqa: E402
from sat_amd import cider as cider_mod  # noqa: E402
from sat_amd import distributed as sat_dist  # noqa: E402
from sat_amd.data import synthetic_captions, synthetic_images  # noqa: E402

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)   # train.py:27-32
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


class AverageMeter:
    """utils.py:4-19"""

    def __init__(self):
        self.val = self.avg = self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count if self.count else 0


class JsonCaptionDataset(torch.utils.data.Dataset):
    """The reference's on-disk layout (generate_json_data.py:51-63, dataset.py:15-52), loaded
    lazily per item (the reference decodes every image eagerly into RAM, which does not fit COCO)."""

    def __init__(self, data_path, split_type="train", fraction=1.0, bert=False, decode_only=False,
                 captions_only=False):
        self.decode_only = decode_only   # uint8 HWC at native size; resize + normalize run on the GPU
        self.captions_only = captions_only   # (row index, caption, all captions): no image is opened (--cache-features)
        self.paths = json.load(open(os.path.join(data_path, f"{split_type}_img_paths.json")))
        name = f"{split_type}_captions_bert.json" if bert else f"{split_type}_captions.json"
        self.captions = json.load(open(os.path.join(data_path, name)))
        if fraction != 1.0:
            self.paths = self.paths[:int(len(self.paths) * fraction)]
            self.captions = self.captions[:int(len(self.captions) * fraction)]
        by_path = {}
        for p, c in zip(self.paths, self.captions):
            by_path.setdefault(p, []).append(c)
        self.all_captions = [by_path[p] for p in self.paths]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        caps = torch.tensor(self.captions[i]), torch.tensor(self.all_captions[i])
        if self.captions_only:
            return (i,) + caps
        from PIL import Image
        with open(self.paths[i], "rb") as f:   # dataset.py:9-12
            img = Image.open(f).convert("RGB")
        if self.decode_only:
            return (np.asarray(img, dtype=np.uint8),) + caps
        img = img.resize((224, 224), Image.BILINEAR)   # host transform (train.py:27-32), --host-preprocess
        x = (np.asarray(img, dtype=np.float32) / 255.0 - MEAN) / STD
        return (torch.from_numpy(x.transpose(2, 0, 1).copy()),) + caps


class SyntheticDataset(torch.utils.data.Dataset):
    def __init__(self, n, vocab, T, bert, seed, captions_only=False):
        g = torch.Generator().manual_seed(seed)
        self.caps = synthetic_captions(n, T, vocab, generator=g, bert=bert)
        self.seed = seed
        self.captions_only = captions_only

    def __len__(self):
        return self.caps.shape[0]

    def __getitem__(self, i):
        if self.captions_only:
            return i, self.caps[i], self.caps[i:i + 1]
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        return synthetic_images(1, generator=g)[0], self.caps[i], self.caps[i:i + 1]


def set_seed(seed):
    """train.py:37-43"""
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def parse(argv=None):
    p = argparse.ArgumentParser(description="Show, Attend and Tell (MI355X)")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--step-size", type=int, default=5)
    p.add_argument("--alpha-c", type=float, default=1)
    p.add_argument("--perform-test", action="store_true", default=True)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--log-interval", type=int, default=100)
    p.add_argument("--data", type=str, default="data/coco")
    p.add_argument("--network", choices=["vgg19", "resnet152", "densenet161"], default="vgg19")
    p.add_argument("--model", type=str)
    p.add_argument("--tf", action="store_true", default=False)
    p.add_argument("--ado", action="store_true", default=False)
    p.add_argument("--fraction", type=float, default=1.0)
    p.add_argument("--bert", action="store_true", default=False)
    p.add_argument("--attention", action="store_true", default=False)
    # MI355X build
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--vocab", type=int, default=10000)
    p.add_argument("--seq", type=int, default=27)
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--max-steps", type=int, default=0)
    p.add_argument("--out", type=str, default="model")
    p.add_argument("--no-overlap", action="store_true",
                   help="encode each batch right before its decoder step instead of one batch ahead on a side stream")
    p.add_argument("--encoder-weights", type=str, default=None,
                   help="torchvision-layout encoder state_dict (weights_only); default: random init under --seed")
    p.add_argument("--host-preprocess", action="store_true",
                   help="resize + normalize on the host workers (default: workers only decode; the GPU resamples "
                        "the uint8 images bit-identically to PIL and normalizes into the encoder's input layout)")
    p.add_argument("--workers", type=int, default=8, help="DataLoader decode workers per rank")
    p.add_argument("--beam-eval", type=int, default=0,
                   help="beam width of an extra generated-caption BLEU in evaluation (0 = off)")
    p.add_argument("--bert-embeddings", type=str, default=None,
                   help="local bert-base-uncased word-embedding table [30522, 768] (weights_only)")
    p.add_argument("--fine-tune-encoder", type=int, default=0,
                   help="train the last N units of the trunk (resnet152: layer4's identity bottlenecks, N <= 2; "
                        "vgg19: the block-5 convolutions, N <= 4); 0 = frozen encoder")
    p.add_argument("--encoder-lr", type=float, default=1e-5, help="Adam learning rate of the trainable encoder units")
    p.add_argument("--cache-features", action="store_true",
                   help="encode every unique image once before epoch 1, keep the frozen trunk's output in HBM and "
                        "train / evaluate from it (with --fine-tune-encoder: the activation entering the tail)")
    p.add_argument("--feature-cache", type=str, default=None, metavar="DIR",
                   help="implies --cache-features; load valid cache files from DIR, write them there after a fill")
    p.add_argument("--tf-prob", type=float, default=None, metavar="P",
                   help="scheduled sampling: while training, every step feeds the ground-truth token with "
                        "probability P and the model's own argmax otherwise (validation / test follow --tf)")
    p.add_argument("--tf-prob-end", type=float, default=None, metavar="Q",
                   help="with --tf-prob: linear decay from P in epoch 1 to Q in the last epoch (default: P)")
    p.add_argument("--scst", action="store_true", default=False,
                   help="self-critical sequence training: sample a caption, score it against the greedy caption's "
                        "reward, follow the policy gradient (start from a cross-entropy checkpoint with --model)")
    p.add_argument("--scst-temperature", type=float, default=1.0, metavar="T",
                   help="with --scst: the temperature of the sampled caption")
    p.add_argument("--scst-reward", choices=["cider", "bleu", "cider-device"], default="cider",
                   help="with --scst: the sentence reward (CIDEr-D over token ids | sentence BLEU-4 | the same CIDEr-D "
                        "scored on the device: no host round trip in the step)")
    p.add_argument("--clip-grad-norm", type=float, default=None, metavar="C",
                   help="clip the gradients to global L2 norm C inside the Adam step, on the device (default: off)")
    args = p.parse_args(argv)
    if args.clip_grad_norm is not None and not 0.0 < args.clip_grad_norm < float("inf"):
        p.error("--clip-grad-norm must be a finite number > 0")
    if args.scst:
        if args.tf or args.tf_prob is not None:
            p.error("--scst samples the fed tokens from the model itself: it cannot be combined with --tf or "
                    "--tf-prob")
        if not args.scst_temperature >= 0.0:
            p.error("--scst-temperature must be >= 0")
    if args.feature_cache:
        args.cache_features = True
    if args.tf_prob is None:
        if args.tf_prob_end is not None:
            p.error("--tf-prob-end needs --tf-prob")
    else:
        if args.tf_prob_end is None:
            args.tf_prob_end = args.tf_prob
        for name, v in (("--tf-prob", args.tf_prob), ("--tf-prob-end", args.tf_prob_end)):
            if not 0.0 <= v <= 1.0:
                p.error(f"{name} must be in [0, 1]")
    return args


def tf_prob_schedule(epoch, epochs, start, end):
    """Teacher probability of ``epoch`` (1-based) of ``epochs``: linear from ``start`` in epoch 1 to ``end`` in the
    last epoch (a single epoch trains at ``start``)."""
    if epochs <= 1 or epoch <= 1:
        return float(start)
    if epoch >= epochs:
        return float(end)
    return float(start + (end - start) * (epoch - 1) / (epochs - 1))


def load_bert_embeddings(path):
    """The frozen BERT word-embedding table the reference takes from BertModel.from_pretrained
    (decoder.py:21-36), from a local file: a tensor or a state_dict holding it."""
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(obj, dict):
        for k in ("embeddings.word_embeddings.weight", "bert.embeddings.word_embeddings.weight",
                  "word_embeddings.weight", "embedding.weight", "weight"):
            if k in obj:
                obj = obj[k]
                break
        else:
            raise ValueError(f"{path}: no word-embedding table among keys {sorted(obj)[:8]}")
    if obj.dim() != 2 or obj.shape[1] != sat_amd.Decoder.BERT_HIDDEN:
        raise ValueError(f"{path}: expected a [V, 768] table, got {tuple(obj.shape)}")
    return obj.float()


def build(args, device):
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    word_dict = None
    if args.bert:
        vocab = sat_amd.Decoder.BERT_VOCAB
    elif args.synthetic:   # generate_json_data.py:45-48 special ids + placeholder words
        vocab = args.vocab
        word_dict = {"<start>": 0, "<eos>": 1, "<unk>": 2, "<pad>": 3}
        word_dict.update({f"w{i}": i for i in range(4, vocab)})
    else:
        word_dict = json.load(open(os.path.join(args.data, "word_dict.json")))
        vocab = len(word_dict)
    encoder = sat_amd.Encoder(args.network, dtype=dt, fine_tune=args.fine_tune_encoder)
    if args.encoder_weights:
        encoder.load_state_dict(torch.load(args.encoder_weights, map_location="cpu", weights_only=True))
    bert_w = None
    if args.bert:
        if args.bert_embeddings:
            bert_w = load_bert_embeddings(args.bert_embeddings)
            vocab = bert_w.shape[0]
        elif not args.model:
            print("WARNING: --bert without --bert-embeddings or --model: the frozen word-embedding table is "
                  "randomly initialised, not bert-base-uncased's (decoder.py:21-36); this is not the reference's "
                  "BERT configuration", file=sys.stderr, flush=True)
    decoder = sat_amd.Decoder(vocab, encoder.dim, tf=args.tf, ado=args.ado, bert=args.bert, attention=args.attention,
                              bert_embedding_weight=bert_w)
    if args.model:   # train.py:65-67 (reference checkpoints load unchanged)
        decoder.load_state_dict(torch.load(args.model, map_location="cpu", weights_only=True))
    return encoder.to(device).eval(), decoder.to(device), word_dict, dt


SPLIT_SEED = {"train": 0, "val": 1, "test": 2}   # fixed per-split offsets (str hash() is randomised per process)


class ShardSampler(torch.utils.data.Sampler):
    """Rank r's items r, r+N, r+2N, ... of an evaluation split: every item exactly once across ranks
    (DistributedSampler pads with repeats), so gathered BLEU / meters cover the whole split."""

    def __init__(self, n, rank, world):
        self.idx = list(range(rank, n, world))

    def __iter__(self):
        return iter(self.idx)

    def __len__(self):
        return len(self.idx)


def make_dataset(args, split, captions_only=False):
    if args.synthetic:
        return SyntheticDataset(args.synthetic if split == "train" else max(args.batch_size, args.synthetic // 8),
                                args.vocab if not args.bert else sat_amd.Decoder.BERT_VOCAB,
                                32 if args.bert else args.seq, args.bert, seed=args.seed * 10 + SPLIT_SEED[split],
                                captions_only=captions_only)
    return JsonCaptionDataset(args.data, split, args.fraction, args.bert, decode_only=not args.host_preprocess,
                              captions_only=captions_only)


def loaders(args, split, rank, world, captions_only=False):
    """The split's loader.  ``captions_only``: its batches are (dataset rows, captions, all captions) and no worker
    opens an image (the features come from a FeatureCache)."""
    ds = make_dataset(args, split, captions_only)
    train = split == "train"
    packed = not args.synthetic and not args.host_preprocess and not captions_only
    if world > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=True, seed=args.seed) \
            if train else ShardSampler(len(ds), rank, world)
    else:
        sampler = None
    # train.py:76-88: the reference shuffles train only and keeps every validation / test batch
    return torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=train and sampler is None,
                                       sampler=sampler,
                                       num_workers=args.workers if not (args.synthetic or captions_only) else 0,
                                       pin_memory=True, drop_last=train,
                                       collate_fn=sat_amd.collate_packed if packed else None)


def encoded_batches(loader, encoder, device, dt, max_steps, overlap):
    """(batch_idx, features, captions) of every training batch.  With ``overlap`` the frozen
    encoder forward (and the host-to-device copy) of batch i+1 is issued on a side stream before
    batch i is handed out, so it runs on the GPU beside batch i's decoder step, all-reduce and
    Adam (the encoder reads no decoder parameter; train.py:29-31 freezes it for VGG19 and the
    reference never optimises ResNet152's)."""
    main = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device) if overlap else main
    # a fine-tuned encoder: only the frozen prefix (plan steps 0 .. tail_start(), which read no trainable weight) runs
    # ahead; the tail runs on the main stream inside the step, after the previous step's update
    k = encoder.tail_start() if getattr(encoder, "_fine_tune", 0) else None

    def encode(imgs, captions):
        with torch.cuda.stream(side), torch.no_grad():
            imgs = imgs.to(device, non_blocking=True)   # a Tensor, or PackedImages (uint8, native size)
            captions = captions.to(device, non_blocking=True)
            feats = encoder(imgs, dtype=dt) if k is None else encoder(imgs, dtype=dt, steps=(0, k))
            ev = torch.cuda.Event()
            ev.record(side)
        return feats, captions, ev

    def tail(batch):
        if k is None:
            return batch
        batch_idx, act, caps = batch
        return batch_idx, encoder(act, dtype=dt, steps=(k, encoder._plan_len())), caps

    pending = None
    for batch_idx, (imgs, captions, _) in enumerate(loader):
        if max_steps and batch_idx >= max_steps:
            break
        nxt = encode(imgs, captions)
        if pending is not None:
            yield tail(pending)
        feats, caps, ev = nxt
        main.wait_event(ev)
        if side is not main:   # produced on the side stream, consumed on the main one
            feats.record_stream(main)
            caps.record_stream(main)
        pending = (batch_idx, feats, caps)
    if pending is not None:
        yield tail(pending)


def preprocess_mode(args):
    """How an image becomes the encoder's input: part of a cache file's key."""
    return "synthetic" if args.synthetic else ("host" if args.host_preprocess else "device")


def build_feature_cache(args, split, encoder, device, dt, rank, world, log):
    """The split's FeatureCache: loaded from --feature-cache DIR when a valid file is there, else filled by one pass
    over the split's unique images (and then written to DIR by rank 0).  Every rank holds the whole cache."""
    t0 = time.time()
    ds = make_dataset(args, split)
    keys = ds.paths if hasattr(ds, "paths") else range(len(ds))
    cache = sat_amd.FeatureCache(encoder, keys, dt, args.batch_size)
    how = "loaded" if args.feature_cache and cache.load(args.feature_cache, split, preprocess_mode(args), device) \
        else "built"
    if how == "built":
        packed = not args.synthetic and not args.host_preprocess
        cache.fill(cache.image_loader(ds, 0 if args.synthetic else args.workers,
                                      sat_amd.collate_packed if packed else None), device)
    if args.feature_cache:
        if world > 1:
            dist.barrier()   # no rank still reads a file rank 0 is about to replace
        if how == "built" and rank == 0:
            cache.save(args.feature_cache, split, preprocess_mode(args))
        if world > 1:
            dist.barrier()
    torch.cuda.synchronize(device)
    log({"feature_cache": how, "split": split, "images": cache.n_images, "bytes": cache.nbytes,
         "seconds": time.time() - t0})
    return cache


def cached_batches(loader, cache, encoder, device, dt, max_steps):
    """(batch_idx, features, captions) of every batch, as encoded_batches yields them, from a captions-only loader
    and a FeatureCache: one gather launch instead of the trunk.  A fine-tuned encoder's cache holds the activation
    entering its tail, which runs here (under the caller's grad mode) as encoded_batches' tail() runs it."""
    k = encoder.tail_start() if getattr(encoder, "_fine_tune", 0) else None
    for batch_idx, (rows, captions, _) in enumerate(loader):
        if max_steps and batch_idx >= max_steps:
            break
        feats = cache.gather(cache.slots[rows])
        captions = captions.to(device, non_blocking=True)
        if k is not None:
            feats = encoder(feats, dtype=dt, steps=(k, encoder._plan_len()))
        yield batch_idx, feats, captions


def clip_record(opt):
    """grad_norm and skipped_steps of the last step for a log line (--clip-grad-norm): one host read."""
    if opt.clip_state is None:
        return {}
    norm, _, _, skipped = opt.clip_state.tolist()
    return dict(grad_norm=norm, skipped_steps=int(skipped))


def train_epoch(epoch, encoder, decoder, opt, loader, args, device, dt, world, log, grad_ar=None, cache=None):
    """train.py:119-192.  ``grad_ar``: a sat_amd.distributed.GradAllReduce for DP (N > 1).  ``cache``: the train
    split's FeatureCache (``loader`` then is the captions-only one)."""
    encoder.eval()
    decoder.train()
    pad, skip = sat_amd.special_ids(args.bert)
    # the reference updates its meters every batch (train.py:179-181) with 4 host syncs per step; here
    # they accumulate on the device and are read once per log line
    meters = sat_amd.RunningMeters(device)
    batches = encoded_batches(loader, encoder, device, dt, args.max_steps, not args.no_overlap) if cache is None \
        else cached_batches(loader, cache, encoder, device, dt, args.max_steps)
    for batch_idx, feats, captions in batches:
        opt.zero_grad()
        preds, alphas = decoder(feats, captions)
        loss, metrics = sat_amd.caption_loss(preds, alphas, captions, args.alpha_c, pad, skip)
        loss.backward()   # with DP the head bucket's all-reduce starts inside it, beside BPTT
        if grad_ar is not None:
            grad_ar.wait()
            if args.fine_tune_encoder:   # the tail's gradients, after the decoder's buckets: ranks must not drift
                sat_dist.all_reduce_tail_grads(encoder)
        opt.step()
        meters.update(loss, metrics)
        if batch_idx % args.log_interval == 0:   # train.py:183-192
            m = meters.read()
            log(dict(epoch=epoch, batch=batch_idx, train_loss=m["loss"], train_top1_acc=m["top1"],
                     train_top5_acc=m["top5"], train_loss_raw=m["loss_val"], train_tokens=m["count"],
                     **clip_record(opt)))
    if cache is not None:
        cache.check_bad_rows()   # the one host read of the gather kernel's bad-row count per epoch
    return meters.read()["loss"] if meters.last is not None else 0.0


class ScstReward:
    """The host reward of --scst: one float per caption (token ids) against the references of its image.  The
    loader's third element, all_captions, only keys the references: CiderD is indexed by image.  With --scst-reward
    cider-device it also holds the corpus on the device (``device_cider``) and the image of every dataset row."""

    def __init__(self, args, dataset, device=None):
        ids = cider_mod.BERT_IDS if args.bert else cider_mod.PLAIN_IDS
        self.ids = (ids["start_id"], ids["end_id"], ids["pad_id"])
        self.kind = args.scst_reward
        if hasattr(dataset, "all_captions"):   # one entry per row; the rows of an image share the list
            seen, refs = {}, []
            for cs in dataset.all_captions:
                key = self._key(cs)
                if key not in seen:
                    seen[key] = len(refs)
                    refs.append(cs)
        else:   # synthetic: one caption per image
            refs = [[c] for c in dataset.caps.tolist()]
            seen = {self._key(r): i for i, r in enumerate(refs)}
        self.index = seen
        self.cider = sat_amd.CiderD(refs, *self.ids)
        self.device_cider = self.row_image = None
        if self.kind == "cider-device":   # the corpus resident on the device, and the image of every dataset row
            self.device_cider = sat_amd.CiderDDevice(self.cider, device)
            rows = dataset.all_captions if hasattr(dataset, "all_captions") else refs
            self.row_image = torch.tensor([seen[self._key(cs)] for cs in rows], dtype=torch.int64, device=device)

    def images(self, all_caps, rows, device):
        """The image index of every row of the batch as an int64 device vector: from the loader's dataset rows when it
        hands them over (--cache-features), else by the host lookup of the rows' reference lists -- which depends on
        nothing the device computed, so neither waits for it."""
        if rows is not None:
            return self.row_image[rows.to(device, non_blocking=True)]
        return torch.tensor([self.index[self._key(r)] for r in all_caps.tolist()], dtype=torch.int64).to(
            device, non_blocking=True)

    @staticmethod
    def _key(refs):
        return tuple(tuple(int(t) for t in r) for r in refs)

    def __call__(self, captions, all_caps):
        images = [self.index[self._key(r)] for r in all_caps]
        if self.kind == "cider":
            return self.cider.score(captions, images)
        strip = lambda c: [str(t) for t in cider_mod.strip_ids(c, *self.ids)]  # noqa: E731
        out = []
        for c, i in zip(captions, images):
            hyp = strip(c)
            out.append(float(bleu_mod.corpus_bleu([[strip(r) for r in self.cider.refs[i]]], [hyp])) if hyp else 0.0)
        return out


def scst_batches(loader, encoder, cache, device, dt, max_steps):
    """(batch_idx, features, all_captions, dataset rows) of every training batch, the trunk (or its cached output) under
    no_grad except for a fine-tuned tail.  The rows are the loader's when it yields them (a cache), else None."""
    k = encoder.tail_start() if getattr(encoder, "_fine_tune", 0) else None
    for batch_idx, (imgs, _, all_caps) in enumerate(loader):
        if max_steps and batch_idx >= max_steps:
            break
        with torch.no_grad():
            if cache is not None:
                feats = cache.gather(cache.slots[imgs])
            elif k is None:
                feats = encoder(imgs.to(device, non_blocking=True), dtype=dt)
            else:
                feats = encoder(imgs.to(device, non_blocking=True), dtype=dt, steps=(0, k))
        if k is not None:
            feats = encoder(feats, dtype=dt, steps=(k, encoder._plan_len()))
        yield batch_idx, feats, all_caps, imgs if cache is not None else None


def scst_epoch(epoch, encoder, decoder, opt, loader, args, device, dt, log, reward, grad_ar=None, cache=None):
    """One epoch of self-critical sequence training.  Per step: a sample-mode forward in train mode, a greedy forward
    under no_grad in eval mode, both token matrices to the host in one copy, the rewards, advantage = r_sample -
    r_greedy, the token-weighted loss, backward, the optimizer step.  With --scst-reward cider-device both token
    matrices are scored where they are (one launch), the advantage is a device subtraction and nothing is copied to the
    host; the reward sums of the log accumulate in a device tensor that is read on --log-interval steps only."""
    encoder.eval()
    end_id = reward.ids[1]
    on_device = reward.device_cider is not None
    sums, n_logged, last = [0.0, 0.0], 0, 0.0
    sums_dev = torch.zeros(2, dtype=torch.float64, device=device) if on_device else None
    for batch_idx, feats, all_caps, rows in scst_batches(loader, encoder, cache, device, dt, args.max_steps):
        B = feats.shape[0]
        steps = all_caps.shape[2] - 1
        if not on_device:
            all_caps = all_caps.tolist()
        opt.zero_grad()
        decoder.train()
        preds, alphas, sampled = decoder.sample(feats, steps, temperature=args.scst_temperature)
        decoder.eval()
        with torch.no_grad():
            greedy = decoder.sample(feats.detach(), steps, temperature=0.0)[2]   # temperature 0: the greedy forward
        decoder.train()
        if on_device:
            images = reward.images(all_caps, rows, device)
            r = reward.device_cider.score(torch.cat([sampled, greedy]), torch.cat([images, images]))
            advantage = r[:B] - r[B:]
        else:
            both = torch.cat([sampled, greedy]).cpu().tolist()   # the one device-to-host copy of the step
            r_sample, r_greedy = reward(both[:B], all_caps), reward(both[B:], all_caps)
            advantage = torch.tensor([a - b for a, b in zip(r_sample, r_greedy)], dtype=torch.float32, device=device)
        w = sat_amd.scst_weights(sampled, advantage, (end_id,))
        loss, logp = sat_amd.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
        loss.backward()
        if grad_ar is not None:
            grad_ar.wait()
            if args.fine_tune_encoder:
                sat_dist.all_reduce_tail_grads(encoder)
        opt.step()
        if on_device:
            sums_dev += r.double().view(2, B).sum(1) / B
        else:
            sums[0] += sum(r_sample) / B
            sums[1] += sum(r_greedy) / B
        n_logged += 1
        if batch_idx % args.log_interval == 0:
            if on_device:
                sums = sums_dev.tolist()
            # the sampled sentences' positions (up to and including the first end token), whatever their advantage
            scored = sat_amd.scst_weights(sampled, torch.full((B,), float(B), device=device), (end_id,))
            mean_logp = float((logp * scored).sum() / scored.sum().clamp_min(1))
            last = float(loss)
            log(dict(epoch=epoch, batch=batch_idx, train_loss=last, scst_reward_sample=sums[0] / n_logged,
                     scst_reward_greedy=sums[1] / n_logged, scst_logp=mean_logp, **clip_record(opt)))
    if cache is not None:
        cache.check_bad_rows()
    if on_device:
        reward.device_cider.check_bad_images()   # one host read per epoch, as the cache's
    return last


def evaluate(epoch, encoder, decoder, loader, args, device, dt, word_dict, mode, log, cache=None):
    """train.py:198-347 (teacher-forced greedy hypotheses, BLEU-1..4); with --beam-eval K also the BLEU of the
    sentences batched beam search generates from the same features.  ``cache``: the split's FeatureCache (``loader``
    then is the captions-only one and its first item the dataset rows)."""
    encoder.eval()
    decoder.eval()
    pad, skip = sat_amd.special_ids(args.bert)
    losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter()
    refs, hyps, beam_hyps = [], [], []
    tok = decoder.tokenizer if args.bert else None
    inv = {i: w for w, i in word_dict.items()} if word_dict else None
    with torch.no_grad():
        for batch_idx, (imgs, captions, all_caps) in enumerate(loader):
            if args.max_steps and batch_idx >= args.max_steps:
                break
            if cache is None:
                imgs, captions = imgs.to(device), captions.to(device)   # Tensor or PackedImages
                feats = encoder(imgs, dtype=dt)
            else:
                captions = captions.to(device)
                feats = cache.gather(cache.slots[imgs])
                if args.fine_tune_encoder:
                    feats = encoder(feats, dtype=dt, steps=(encoder.tail_start(), encoder._plan_len()))
            preds, alphas = decoder(feats, captions)
            loss, metrics = sat_amd.caption_loss(preds, alphas, captions, args.alpha_c, pad, skip)
            m = sat_amd.StepMetrics(loss, metrics).values()
            n = m["caption_length"]
            losses.update(m["loss"], n); top1.update(m["acc1"], n); top5.update(m["acc5"], n)
            ids = preds.argmax(dim=2).cpu().tolist()
            if args.bert:
                dec = lambda c: bleu_mod.decode_bert(c, tok)  # noqa: E731
            elif word_dict:
                dec = lambda c: bleu_mod.decode_plain(c, word_dict, inv)  # noqa: E731
            else:
                dec = lambda c: [str(t) for t in c if t not in (0, 3)][:c.index(1) if 1 in c else None]  # noqa: E731
            refs += [[dec(c) for c in cs] for cs in all_caps.tolist()]
            hyps += [dec(c) for c in ids]
            if args.beam_eval > 0:
                with contextlib.redirect_stdout(sys.stderr):   # the "no completed sentence" notices: not JSON
                    beam_hyps += [dec(s) for s, _, _ in decoder.caption_batch(feats, args.beam_eval)]
    sums = [losses.sum, top1.sum, top5.sum, losses.count]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        # every rank evaluated a disjoint shard (ShardSampler): gather hypotheses, references and the
        # meters' sums so the logged BLEU-1..4 and averages cover the whole split
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, (refs, hyps, sums, beam_hyps))
        refs = [r for p in parts for r in p[0]]
        hyps = [h for p in parts for h in p[1]]
        sums = [sum(p[2][i] for p in parts) for i in range(4)]
        beam_hyps = [h for p in parts for h in p[3]]
    n = sums[3]
    avg = [v / n if n else 0.0 for v in sums[:3]]
    b1, b2, b3, b4 = bleu_mod.bleu_1_to_4(refs, hyps)
    if cache is not None:
        cache.check_bad_rows()
    rec = {"epoch": epoch, f"{mode}_loss": avg[0], f"{mode}_top1_acc": avg[1], f"{mode}_top5_acc": avg[2],
           f"{mode}_bleu1": b1, f"{mode}_bleu2": b2, f"{mode}_bleu3": b3, f"{mode}_bleu4": b4}
    if args.beam_eval > 0:
        for i, b in enumerate(bleu_mod.bleu_1_to_4(refs, beam_hyps), 1):
            rec[f"{mode}_beam_bleu{i}"] = float(b)
    log(rec)
    return b4


def main(argv=None):
    args = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    device = torch.device("cuda", local)
    set_seed(args.seed)

    def log(rec):
        if rank == 0:
            print(json.dumps(rec), flush=True)

    if args.scst and not args.model:
        print("WARNING: --scst without --model: self-critical training is the stage after cross-entropy training and "
              "starts here from a randomly initialised decoder", file=sys.stderr, flush=True)
    encoder, decoder, word_dict, dt = build(args, device)
    decoder.record_tokens = False   # no fed-token record per training step
    if not args.no_overlap:   # the decoder shares the chip with the next batch's encoder (bench.py defaults)
        decoder.split_target = 128 if args.network == "vgg19" else (96 if args.batch_size > 64 else 64)   # as bench.py
        # no layer3 block fused: the unfused c2 / c3 half-image kernels leave CUs to the decoder
        # (profiles/r2_s62_sched.txt)
        encoder.fuse_blocks = False
    if args.fine_tune_encoder:   # the tail's parameters as a second param group (one launch per tensor)
        opt = sat_amd.Adam([{"params": list(decoder.parameters())},
                            {"params": encoder.tail_parameters(), "lr": args.encoder_lr}], lr=args.lr,
                           max_grad_norm=args.clip_grad_norm)
    else:
        opt = sat_amd.Adam(decoder.parameters(), lr=args.lr, max_grad_norm=args.clip_grad_norm)
    grad_ar = sat_dist.GradAllReduce(decoder) if world > 1 else None
    sched = torch.optim.lr_scheduler.StepLR(opt, args.step_size)
    caches = {}
    if args.cache_features:   # one pre-pass over each split's unique images (or a load), then loaders without images
        for split in ("train", "val") + (("test",) if args.perform_test else ()):
            caches[split] = build_feature_cache(args, split, encoder, device, dt, rank, world, log)
    train_loader = loaders(args, "train", rank, world, captions_only=args.cache_features)
    val_loader = loaders(args, "val", rank, world, captions_only=args.cache_features)
    reward = ScstReward(args, train_loader.dataset, device) if args.scst else None
    os.makedirs(args.out, exist_ok=True)
    enc_path = os.path.join(args.out, f"encoder_{args.network}.pth")
    if rank == 0:   # the trunk this run uses, so generate_caption.py encodes with the same weights
        torch.save({k: v.detach().cpu() for k, v in encoder.state_dict().items()}, enc_path)
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        if isinstance(getattr(train_loader, "sampler", None), torch.utils.data.distributed.DistributedSampler):
            train_loader.sampler.set_epoch(epoch)
        if args.tf_prob is not None:   # scheduled sampling: set once per epoch (eval mode ignores it)
            decoder.tf_prob = tf_prob_schedule(epoch, args.epochs, args.tf_prob, args.tf_prob_end)
        if args.scst:
            scst_epoch(epoch, encoder, decoder, opt, train_loader, args, device, dt, log, reward, grad_ar,
                       caches.get("train"))
        else:
            train_epoch(epoch, encoder, decoder, opt, train_loader, args, device, dt, world, log, grad_ar,
                        caches.get("train"))
        evaluate(epoch, encoder, decoder, val_loader, args, device, dt, word_dict, "val", log, caches.get("val"))
        sched.step()
        if rank == 0:   # train.py:103-110
            torch.save(decoder.state_dict(), os.path.join(args.out, f"model_{args.network}_{epoch}.pth"))
            cfg = dict(vars(args))
            cfg["encoder_weights"] = os.path.abspath(enc_path)
            if args.fine_tune_encoder:   # the tuned trunk of this epoch, beside the decoder's checkpoint
                tuned = os.path.join(args.out, f"encoder_{args.network}_{epoch}.pth")
                torch.save({k: v.detach().cpu() for k, v in encoder.state_dict().items()}, tuned)
                cfg["encoder_weights"] = os.path.abspath(tuned)
            if args.synthetic and word_dict:   # generate_caption.py reads <data>/word_dict.json
                cfg["data"] = args.out
                with open(os.path.join(args.out, "word_dict.json"), "w") as f:
                    json.dump(word_dict, f)
            with open(os.path.join(args.out, "model_config.json"), "w") as f:
                json.dump(cfg, f)
        rec = {"epoch": epoch, "epoch_seconds": time.time() - t0}
        if args.tf_prob is not None:
            rec["tf_prob"] = decoder.tf_prob
        log(rec)
    if args.perform_test:
        test_loader = loaders(args, "test", rank, world, captions_only=args.cache_features)
        evaluate(args.epochs, encoder, decoder, test_loader, args, device, dt, word_dict, "test", log,
                 caches.get("test"))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
