// What a batch with log-probabilities switched on launches behind a pick (metalchat_amd/csrc/batch_plan.h plan_logprobs / check_logprobs, Part 2n of the
// ABI) from the command line, without HIP: one request per line of standard input, one line of JSON per answer.  A launch is answered as [name, gx,
// gy, gz, block, lds], a refusal as {"refused": "<text>"}.
//
//     plan   enabled top_n vocab rows ragged   -> {"any": false} or {"any": true, "nchunk": n, "parts": launch, "finish": launch} or the refusal
//     set    enable top_n vocab                -> {"ok": true} or the refusal
//     abi                                      -> {"max_top", "threads", "chunk", "key_cap", "part_bytes"}
//
// tests/test_logprobs_cpu.py asks.
#include "../../metalchat_amd/csrc/batch_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>

using namespace mcimpl;

static std::string
js(const launch_plan& l)
{
    return "[\"" + l.name + "\", " + std::to_string(l.gx) + ", " + std::to_string(l.gy) + ", " + std::to_string(l.gz) + ", " + std::to_string(l.block) + ", " +
           std::to_string(l.lds) + "]";
}

static std::string
refused(const std::string& why)
{
    return "{\"refused\": \"" + why + "\"}";
}

int
main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "plan") {
            int enabled = 0, top_n = 0, vocab = 0, rows = 0, ragged = 0;
            if (!(in >> enabled >> top_n >> vocab >> rows >> ragged)) return 2;
            const logprobs_plan p = plan_logprobs(enabled != 0, top_n, vocab, rows, ragged != 0);
            if (!p.refusal.empty()) puts(refused(p.refusal).c_str());
            else if (!p.any) puts("{\"any\": false}");
            else
                puts(("{\"any\": true, \"nchunk\": " + std::to_string(p.nchunk) + ", \"parts\": " + js(p.parts) + ", \"finish\": " + js(p.finish) + "}").c_str());
        } else if (what == "set") {
            int enable = 0, top_n = 0, vocab = 0;
            if (!(in >> enable >> top_n >> vocab)) return 2;
            const std::string why = check_logprobs(enable, top_n, vocab);
            puts(why.empty() ? "{\"ok\": true}" : refused(why).c_str());
        } else if (what == "abi") {
            printf("{\"max_top\": %d, \"threads\": %u, \"chunk\": %u, \"key_cap\": %u, \"part_bytes\": %zu}\n", LOGPROBS_MAX_TOP, LOGPROB_THREADS, LOGPROB_CHUNK,
                   LOGPROB_KEY_CAP, sizeof(logprob_part));
        } else
            return 2;
    }
    return 0;
}
