#!/bin/bash
# rcgan on CIFAR-100 (100 fine labels; --coarse_labels: 20), alpha = 0.6, one MI355X.  Data: ../data/cifar100/cifar-100-python
# Multi-GPU: NGPUS=8 ./run_rcgan_cifar100.sh starts one rank per GPU (RCCL gradient all-reduce).
out=rcgan_cifar100
run_id=0
alpha=0.6
ngpus=${NGPUS:-1}
mkdir -p "$out"
log="$out/rcgan_alpha${alpha}_${run_id}_log.txt"
launch="python"
if [ "$ngpus" -gt 1 ]; then
  launch="python -m torch.distributed.run --nnodes=1 --nproc-per-node $ngpus --master-addr 127.0.0.1"
fi
$launch gan_resnet.py --dataset cifar100 --algorithm rcgan --alpha $alpha --run $run_id \
  --log_file "$log" --parent_dir "$out" --ngpus $ngpus --multi_gpu_multi_batch "$@"
