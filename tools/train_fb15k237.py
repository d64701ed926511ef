"""End-to-end training run of the headline configuration on one MI355X, reporting filtered MRR / HITS:
FB15k-237 + RotatE hidden_dim=1000, K=256, batch 1024, Adversarial alpha=1, gamma=9, Adam.

    python tools/train_fb15k237.py [--epochs 200] [--lr 5e-5] [--eval-every 50] [--model RotatE]
                                   [--loss adversarial|margin|pairwise|softmax|onevsall|kvsall] [--reg none|l2|n3] [--reg-weight 1e-3]
                                   [--optimizer adam|adagrad] [--label-smoothing 0.1] [--filter-known]
                                   [--sampler uniform|weighted|inbatch] [--sampler-power 0.75]
                                   [--relation-prediction LAMBDA] [--relation-temperature T]

--loss: adversarial (the default: Adversarial(--alpha) through FusedTrainStep), margin (MarginRanking(--gamma as the margin,
--alpha)), pairwise (PairwiseLogistic(0, --alpha)) or softmax (CrossEntropy(--temperature)), the last three through
PooledLossStep, or onevsall (OneVsAll(--temperature) through OneVsAllStep: ComplEx / DistMult, every entity scored for each row, no
negatives drawn; --size is then not used; --label-smoothing, and --filter-known to take a row's other known answers in the
training triples out of its softmax), or kvsall (KvsAllStep: the same two models, binary cross entropy against the multi-hot
labels of every known answer in the training triples, --label-smoothing, --reduction mean|sum over the entities); with --model
TransE / RotatE / pRotatE both go through DistanceAllStep, same flags.  --reg: an L2 / N3 penalty of --reg-weight on the rows of each batch's positive triples (regularizers.L2 / N3),
handed to the step.  --optimizer: adam (the default: row-lazy optim.Adam) or adagrad (row-sparse optim.Adagrad; the literature's
ComplEx / DistMult recipe is --loss softmax --reg n3 --optimizer adagrad --lr 0.1), both at --lr.  --sampler: uniform (the default:
sampling.NegativeSampling, the reference's negatives), weighted (sampling.WeightedNegativeSampling: pool entries drawn with probability
proportional to the entity's degree in the training triples to the power --sampler-power) or inbatch
(sampling.InBatchNegativeSampling: the pool is 2 * --size of the batch's own tails / heads).  --relation-prediction LAMBDA: the
auxiliary term losses.RelationPrediction(LAMBDA, --relation-temperature), -log P(r | h, t) over all relations, handed to the step.

Uses the public mkb_amd API only (models / sampling / losses / compose.Pipeline-equivalent loop / evaluation) plus
the device batch producer.  Prints one JSON line per evaluation."""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, evaluation, losses, models, optim, regularizers, sampling  # noqa: E402
from mkb_amd.fused import DISTANCE_MODELS, DistanceAllStep, FusedTrainStep, KvsAllStep, OneVsAllStep, PooledLossStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--eval-every", type=int, default=50)
    ap.add_argument("--model", default="RotatE")
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--gamma", type=float, default=9.0)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dataset", default="Fb15k237")
    ap.add_argument("--loss", default="adversarial", choices=["adversarial", "margin", "pairwise", "softmax", "onevsall", "kvsall"])
    ap.add_argument("--temperature", type=float, default=1.0, help="--loss softmax / onevsall")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="--loss onevsall / kvsall")
    ap.add_argument("--filter-known", action="store_true", help="--loss onevsall: filter a row's other known training answers")
    ap.add_argument("--reduction", default="mean", choices=["mean", "sum"], help="--loss kvsall: over the entities of a row")
    ap.add_argument("--reg", default="none", choices=["none", "l2", "n3"])
    ap.add_argument("--reg-weight", type=float, default=1e-3, help="--reg l2 / n3")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "adagrad"], help="optim.Adam(lazy_rows=True) or optim.Adagrad at --lr")
    ap.add_argument("--sampler", default="uniform", choices=["uniform", "weighted", "inbatch"])
    ap.add_argument("--sampler-power", type=float, default=0.75, help="--sampler weighted: p_e proportional to degree_e ** power")
    ap.add_argument("--relation-prediction", type=float, default=None, metavar="LAMBDA",
                    help="add losses.RelationPrediction(LAMBDA, --relation-temperature) to every step")
    ap.add_argument("--relation-temperature", type=float, default=1.0)
    ap.add_argument("--no-defer", action="store_true", help="apply the optimizer step at once (one more launch per step)")
    args = ap.parse_args()

    ds = getattr(datasets, args.dataset)(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    batches = datasets.DeviceBatches(ds, "cuda", seed=42)
    torch.manual_seed(42)
    model = getattr(models, args.model)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations,
                                        gamma=args.gamma).cuda()
    sampler_args = dict(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
    if args.sampler == "weighted":
        sampler = sampling.WeightedNegativeSampling(weights="degree", power=args.sampler_power, **sampler_args)
    elif args.sampler == "inbatch":
        sampler = sampling.InBatchNegativeSampling(**sampler_args)
    else:
        sampler = sampling.NegativeSampling(**sampler_args)
    ahead = sampler if args.sampler == "uniform" else None  # (only the uniform sampler's draw can ride the optimizer's launch)
    if args.optimizer == "adagrad":  # row-sparse: nothing is deferred, --no-defer has nothing to switch off
        opt = optim.Adagrad([p for p in model.parameters() if p.requires_grad], lr=args.lr, draw_ahead=ahead)
    else:
        opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=args.lr, lazy_rows=True, draw_ahead=ahead,
                         defer_step=not args.no_defer)  # gradients are cleared through opt.zero_grad() only: the step may wait
    reg = {"none": lambda: None, "l2": lambda: regularizers.L2(args.reg_weight), "n3": lambda: regularizers.N3(args.reg_weight)}[args.reg]()
    rp = None if args.relation_prediction is None else losses.RelationPrediction(args.relation_prediction, args.relation_temperature)
    if args.loss == "adversarial":
        step = FusedTrainStep(model, args.alpha, regularizer=reg, relation_prediction=rp)
    elif args.loss in ("onevsall", "kvsall") and args.model in DISTANCE_MODELS:  # the same flags, the distance models' step
        marker = (losses.OneVsAll(args.temperature, args.label_smoothing, args.filter_known) if args.loss == "onevsall"
                  else losses.KvsAll(label_smoothing=args.label_smoothing, reduction=args.reduction))
        step = DistanceAllStep(model, marker, regularizer=reg, true_triples=ds.train, relation_prediction=rp)
    elif args.loss == "onevsall":
        step = OneVsAllStep(model, temperature=args.temperature, regularizer=reg, label_smoothing=args.label_smoothing,
                            true_triples=ds.train if args.filter_known else None, relation_prediction=rp)
    elif args.loss == "kvsall":
        step = KvsAllStep(model, ds.train, label_smoothing=args.label_smoothing, reduction=args.reduction, regularizer=reg, relation_prediction=rp)
    else:
        step = PooledLossStep(model, {"margin": lambda: losses.MarginRanking(margin=args.gamma, alpha=args.alpha),
                                      "pairwise": lambda: losses.PairwiseLogistic(margin=0.0, alpha=args.alpha),
                                      "softmax": lambda: losses.CrossEntropy(temperature=args.temperature)}[args.loss](),
                              regularizer=reg, relation_prediction=rp)
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations,
                               batch_size=1024, device="cuda", num_workers=0)
    n_steps, t_train = 0, 0.0
    for epoch in range(args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for data in batches:
            loss = step.sampled(data["sample"], data["weight"], sampler, data["mode"])
            opt.step()
            opt.zero_grad()
            n_steps += 1
        torch.cuda.synchronize()
        t_train += time.perf_counter() - t0
        sampler.check()
        if (epoch + 1) % args.eval_every == 0 or epoch + 1 == args.epochs:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            valid = ev.eval(model=model, dataset=ds.valid)
            test = ev.eval(model=model, dataset=ds.test)
            torch.cuda.synchronize()
            print(json.dumps({"epoch": epoch + 1, "steps": n_steps, "loss": float(loss.item()),
                              "train_seconds": round(t_train, 2),
                              "triples_per_s": round(n_steps * args.batch * ((len(ds.entities) if args.loss in ("onevsall", "kvsall") else args.size) + 1)
                                                     / t_train),
                              "eval_seconds": round(time.perf_counter() - t1, 2), "valid": valid, "test": test}), flush=True)


if __name__ == "__main__":
    main()
