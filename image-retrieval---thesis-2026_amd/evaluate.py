"""evaluate(model, loader, device, args): drop-in for the reference's hot loop
(test.py:1065-1126; twin test_nonclip.py:132-172).

Same stages, prints and .npz fields -- embed loop -> scores -> self-exclusion -> R@K -> full
ranking -> mAP / mP@K -> majority-vote classification -> np.savez -- but the N x N distance
matrix, topk and argsort of the reference are replaced by one device-resident index and
libmirx's exact full ranking (fp64 scores, ties -> lowest index).
"""
import os

import numpy as np
import torch

from .index import FlatIndex
from .metrics import (_label_bitmasks, compute_classification_metrics, compute_map, compute_map_multilabel, group_codes,
                      map_from_device_result, retrieval_accuracy)

# evaluate() / evaluate_multilabels() keep the [N, N] ranking (result["ranks"], the .npz's dists) up to this many images;
# larger sets, and every call with args.groups, are evaluated by the streaming core, which never builds it
FULL_RANKING_MAX_IMAGES = 65536


@torch.no_grad()
def embed_loader(model, loader, device):
    """test.py:1070-1078: forward every batch, concatenate embeddings and labels on `device`."""
    model.eval()
    embeds, labels = [], []
    for data in loader:
        out = model(data[0].to(device))
        if isinstance(out, dict):
            out = out["embedding"]
        elif isinstance(out, tuple):
            out = out[0]
        embeds.append(out)
        labels.append(data[1].to(device))
    return torch.cat(embeds, dim=0), torch.cat(labels, dim=0)


def rank_self(embeds, metric="cdist"):
    """Self-retrieval ranking of a [N,D] embedding set on its GPU.
    -> (ranks [N,N] int64 row-per-query, self last; reported scores [N,N] in rank order)."""
    n, d = embeds.shape
    ix = FlatIndex(d, "L2" if metric in ("cdist", "L2", "l2") else "COSINE", embeds.device.index or 0)
    ix.add(embeds)
    me = torch.arange(n, device=embeds.device)
    return ix.rank_all(embeds, exclude_ids=me, with_scores=True)


def _self_index(embeds, metric):
    ix = FlatIndex(embeds.shape[1], "L2" if metric in ("cdist", "L2", "l2") else "COSINE", embeds.device.index or 0)
    ix.add(embeds)
    return ix


def _self_heads(ix, embeds, k, codes=None, chunk=8192):
    """The first k entries of every image's own list, itself (and with codes its group) left out: ids [N, k], -1 past
    the eligible rows."""
    n = embeds.shape[0]
    k = min(int(k), n)
    out = []
    for s in range(0, n, chunk):
        me = torch.arange(s, min(s + chunk, n), device=embeds.device)
        if codes is None:
            out.append(ix.search(embeds[s:s + chunk], k, exclude_ids=me)[1])
        else:
            out.append(ix.search_leave_out(embeds[s:s + chunk], k, codes, codes[s:s + chunk], exclude_ids=me)[1])
    return torch.cat(out, dim=0)


def evaluate_embeddings(embeds, labels, groups=None, metric="cdist", kappas=(1, 5, 10), k_values=(1, 5, 10, 15, 20)):
    """The numbers of evaluate() for a [N, D] embedding set on its GPU with [N] class labels, without the [N, N] ranking:
    mAP / mP@K / R@K from FlatIndex.rank_metrics (the full ranking is walked inside the sort's workspace), the
    majority-vote heads from the top max(k_values) of FlatIndex.search.  groups (one value per image, e.g. the patient
    of a study; strings or ints): every image's list loses the images of its own group, itself included, before anything
    is counted -- leave-one-patient-out.  Without groups the numbers are evaluate()'s.
    -> {"acc": R@K percent float32 [len(kappas)], "mAP", "pr": mP@K [len(kappas)], "classification": {k: {...}},
    "n_queries", "n_skipped": images without a relevant image left (AP NaN, skipped in the means)}."""
    if not (torch.is_tensor(embeds) and embeds.is_cuda and embeds.dim() == 2):
        raise ValueError("evaluate_embeddings: embeds must be a [N, D] tensor on a GPU")
    embeds = embeds.float().contiguous()
    n = embeds.shape[0]
    kappas, k_values = [int(k) for k in kappas], [int(k) for k in k_values]
    labels_np = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if labels_np.ndim != 1 or labels_np.shape[0] != n:
        raise ValueError(f"evaluate_embeddings: labels needs one class per image ({n}), got shape {tuple(labels_np.shape)}")
    codes = None if groups is None else torch.from_numpy(group_codes(groups, n)).to(embeds.device)
    lab = torch.as_tensor(labels_np).to(device=embeds.device, dtype=torch.int64)
    ix = _self_index(embeds, metric)
    me = torch.arange(n, device=embeds.device)
    # self_kind 0: without groups the image itself is the positive at the last rank (test.py:119); with groups it carries
    # its own code and leaves with its group
    res = ix.rank_metrics(embeds, lab, lab, kappas, exclude_ids=me, self_kind=0, row_codes=codes, query_codes=codes)
    mAP, aps, pr, _ = map_from_device_result(res, kappas)
    hit = (res["cnt"] > 0).sum(dim=0).cpu().numpy()
    accuracy = np.array([np.float32(np.float32(h) * np.float32(100.0 / n)) for h in hit], dtype=np.float32)
    heads = _self_heads(ix, embeds, max(k_values), codes).cpu().numpy()
    if groups is None:                                                # fewer than k other images: the image itself is the
        heads = np.where(heads < 0, np.arange(n)[:, None], heads)     # last entry of its list, as in the full ranking
    classification = compute_classification_metrics(labels_np, None, k_values, ranks=heads.T, groups=groups)
    return {"acc": accuracy, "mAP": mAP, "pr": pr, "classification": classification, "n_queries": n,
            "n_skipped": int(np.isnan(aps).sum())}


def _print_classification(classification_results, k_values):
    for k in k_values:
        m = classification_results[k]
        print(f"\n>> Top-{k} Retrieved Images:")
        print(f'   Accuracy: {m["accuracy"]:.2f}%')
        print(f'   Precision (macro): {m["precision_macro"]:.2f}%')
        print(f'   Recall (macro): {m["recall_macro"]:.2f}%')
        print(f'   F1 (macro): {m["f1_macro"]:.2f}%')
        print(f'   Precision (weighted): {m["precision_weighted"]:.2f}%')
        print(f'   Recall (weighted): {m["recall_weighted"]:.2f}%')
        print(f'   F1 (weighted): {m["f1_weighted"]:.2f}%')


def _evaluate_streaming(embeds, labels, metric, groups, args):
    """evaluate() past FULL_RANKING_MAX_IMAGES or with args.groups: the same prints, result keys and .npz fields from
    evaluate_embeddings; result["ranks"] is None, and dists is saved only while the [N, N] matrix is allowed."""
    kappas, k_values = [1, 5, 10], [1, 5, 10, 15, 20]
    labels_np = labels.cpu().numpy()
    r = evaluate_embeddings(embeds, labels_np, groups, metric, kappas, k_values)
    accuracy, mAP, pr, classification_results = r["acc"], r["mAP"], r["pr"], r["classification"]
    print(">> R@K{}: {}%".format(kappas, np.around(accuracy, 2)))
    print(">> mAP: {:.2f}%".format(mAP * 100.0))
    print(">> mP@K{}: {}%".format(kappas, np.around(pr * 100.0, 2)))
    print("\n>> Classification Metrics (Majority Voting):")
    _print_classification(classification_results, k_values)
    result = {"embeds": embeds, "labels": labels, "ranks": None, "acc": accuracy, "mAP": mAP, "pr": pr,
              "classification": classification_results, "n_skipped": r["n_skipped"]}
    if getattr(args, "save_dir", None):
        os.makedirs(args.save_dir, exist_ok=True)
        file_name = args.resume.split("/")[-1].split(".")[0]
        save_path = os.path.join(args.save_dir, file_name)
        extra = {}
        n = embeds.shape[0]
        if n <= FULL_RANKING_MAX_IMAGES:                              # as evaluate() builds it; groups do not enter
            ranks, sorted_scores = rank_self(embeds.float(), metric)
            dists = torch.empty((n, n), dtype=torch.float32, device=ranks.device)
            dists.scatter_(1, ranks, -sorted_scores)
            dists.fill_diagonal_(float("inf"))
            extra["dists"] = dists.cpu().numpy()
        np.savez(save_path, embeds=embeds.cpu().numpy(), labels=labels_np, kappas=kappas, acc=accuracy, mAP=mAP, pr=pr,
                 classification_k_values=list(classification_results.keys()),
                 **{f"classification_k{k}": np.array(list(v.values())) for k, v in classification_results.items()}, **extra)
    return result


@torch.no_grad()
def evaluate(model, loader, device, args):
    """args.groups (optional: one value per image of the loader, in its order, e.g. the patient id) makes every number
    leave-group-out; with it, or past FULL_RANKING_MAX_IMAGES images, the streaming core runs and result["ranks"] is None."""
    embeds, labels = embed_loader(model, loader, device)
    metric = getattr(args, "metric", "cdist")
    groups = getattr(args, "groups", None)
    if groups is not None or embeds.shape[0] > FULL_RANKING_MAX_IMAGES:
        return _evaluate_streaming(embeds, labels, metric, groups, args)
    ranks, sorted_scores = rank_self(embeds.float(), metric)
    labels_np = labels.cpu().numpy()
    k_values = [1, 5, 10, 15, 20]
    # only the heads of the lists leave the GPU; AP / precision@k run over the full ranking on the
    # device (mirx_rank_metrics) -- no N x N matrix crosses PCIe
    ranks_head = ranks[:, :max(k_values)].cpu().numpy()

    kappas = [1, 5, 10]
    accuracy = retrieval_accuracy(None, labels_np, topk=kappas, topk_ids=ranks_head[:, :max(kappas)])
    accuracy = torch.stack(accuracy).cpu().numpy()
    print(">> R@K{}: {}%".format(kappas, np.around(accuracy, 2)))

    mAP, _, pr, _ = compute_map(ranks.t(), labels_np, kappas)
    print(">> mAP: {:.2f}%".format(mAP * 100.0))
    print(">> mP@K{}: {}%".format(kappas, np.around(pr * 100.0, 2)))

    print("\n>> Classification Metrics (Majority Voting):")
    classification_results = compute_classification_metrics(labels_np, None, k_values, ranks=ranks_head.T)
    for k in k_values:
        m = classification_results[k]
        print(f"\n>> Top-{k} Retrieved Images:")
        print(f'   Accuracy: {m["accuracy"]:.2f}%')
        print(f'   Precision (macro): {m["precision_macro"]:.2f}%')
        print(f'   Recall (macro): {m["recall_macro"]:.2f}%')
        print(f'   F1 (macro): {m["f1_macro"]:.2f}%')
        print(f'   Precision (weighted): {m["precision_weighted"]:.2f}%')
        print(f'   Recall (weighted): {m["recall_weighted"]:.2f}%')
        print(f'   F1 (weighted): {m["f1_weighted"]:.2f}%')

    result = {"embeds": embeds, "labels": labels, "ranks": ranks, "acc": accuracy, "mAP": mAP, "pr": pr,
              "classification": classification_results}
    if getattr(args, "save_dir", None):
        os.makedirs(args.save_dir, exist_ok=True)
        file_name = args.resume.split("/")[-1].split(".")[0]
        save_path = os.path.join(args.save_dir, file_name)
        # test.py:1124 saves dists = -(-cdist) = +L2 with a +inf diagonal (cosine: -similarity)
        n = ranks.shape[0]
        dists = torch.empty((n, n), dtype=torch.float32, device=ranks.device)
        dists.scatter_(1, ranks, -sorted_scores)
        dists.fill_diagonal_(float("inf"))
        np.savez(save_path, embeds=embeds.cpu().numpy(), labels=labels_np, dists=dists.cpu().numpy(),
                 kappas=kappas, acc=accuracy, mAP=mAP, pr=pr,
                 classification_k_values=list(classification_results.keys()),
                 **{f"classification_k{k}": np.array(list(v.values())) for k, v in classification_results.items()})
    return result


@torch.no_grad()
def evaluate_multilabels(model, loader, device, args):
    """test.py:987-1062 (VinDr-CXR style multi-hot labels): embed loop -> cosine similarities with the diagonal excluded
    -> mAP at Jaccard > 0.25 and > 0.5 (compute_map_multilabel) -> Precision@K (share of the top K with at least one label
    in common with the query) and Recall@K (1 if any of the top K shares a label) for K in 1, 5, 10, 15, 20 -> optional
    np.savez(embeds, labels).  Same prints; returns the numbers (the reference returns None).  The N x N matrix, its
    two argsorts and the Python double loop are replaced by one resident index, one exact full ranking and tensor ops on
    the device."""
    embeds, labels = embed_loader(model, loader, device)
    embeds_norm = torch.nn.functional.normalize(embeds.float(), p=2, dim=1)
    groups = getattr(args, "groups", None)
    streaming = groups is not None or embeds.shape[0] > FULL_RANKING_MAX_IMAGES
    k_values = [1, 5, 10, 15, 20]
    print("\n--- VinDr-CXR Retrieval Results ---")
    out = {"mAP": {}, "precision": {}, "recall": {}}
    if streaming:
        # args.groups (one value per image), or more images than an [N, N] ranking is built for: the full ranking is
        # walked inside the sort's workspace (FlatIndex.rank_metrics) and the heads come from the top-k search
        n = embeds_norm.shape[0]
        masks = _label_bitmasks(labels)
        if masks is None:
            raise ValueError("evaluate_multilabels: the streaming evaluation needs multi-hot 0/1 labels of at most 63 classes")
        codes = None if groups is None else torch.from_numpy(group_codes(groups, n)).to(embeds_norm.device)
        ix = _self_index(embeds_norm.contiguous(), "cosine")
        mt = torch.from_numpy(masks).to(embeds_norm.device)
        me = torch.arange(n, device=embeds_norm.device)
        for t in [0.25, 0.5]:
            aps = ix.rank_metrics(embeds_norm, mt, mt, (), exclude_ids=me, self_kind=1, row_codes=codes, query_codes=codes,
                                  jaccard_threshold=t, standard_ap=True)["ap"].cpu().numpy()
            aps = aps[~np.isnan(aps)]
            m = np.mean(aps) if aps.size else 0
            out["mAP"][t] = float(m)
            print(f">> mAP (Jaccard > {t}): {m * 100.0:.2f}%")
        top = _self_heads(ix, embeds_norm, max(k_values), codes)
        lab = labels.to(top.device).float()
        matches = ((lab[top.clamp(min=0)] * lab[:, None, :]).sum(dim=2) > 0) & (top >= 0)
    else:
        ranks, _ = rank_self(embeds_norm, "cosine")                   # [N, N] row per query, self last
        for t in [0.25, 0.5]:
            m = compute_map_multilabel(None, labels, threshold=t, ranks=ranks.t())
            out["mAP"][t] = float(m)
            print(f">> mAP (Jaccard > {t}): {m * 100.0:.2f}%")
        lab = labels.to(ranks.device).float()
        top = ranks[:, :max(k_values)]
        matches = (lab[top] * lab[:, None, :]).sum(dim=2) > 0          # [N, maxk]: shares a label with the query
    print(f'\n{"K":<5} | {"Precision@K":<15} | {"Recall@K":<15}')
    print("-" * 40)
    n = lab.shape[0]
    for k in k_values:
        cnt = matches[:, :k].sum(dim=1)
        avg_precision = float((cnt.double() / k).sum() / n * 100)
        avg_recall = float((cnt > 0).double().sum() / n * 100)
        out["precision"][k], out["recall"][k] = avg_precision, avg_recall
        print(f"{k:<5} | {avg_precision:<15.2f}% | {avg_recall:<15.2f}%")
    if getattr(args, "save_dir", None):
        os.makedirs(args.save_dir, exist_ok=True)
        save_path = os.path.join(args.save_dir, "evaluation_results.npz")
        np.savez(save_path, embeds=embeds.cpu().numpy(), labels=labels.cpu().numpy())
        print(f"\n>> Results saved to {save_path}")
    return out
