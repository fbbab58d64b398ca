# tools/polyte_time.py under a time limit; prints its one JSON line (arguments are passed on: --pairs N --runs K --out DIR)
set -e -o pipefail
export PYTHONUNBUFFERED=1
timeout -k 10 280 python -u tools/polyte_time.py "$@"
