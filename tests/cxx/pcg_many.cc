// solver::pcg_many of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_pcg_many.py: a 27-point solver
// with room for three right-hand sides (solver.max-rhs in config.json) runs conjugate gradients on all three in lockstep,
// then pcg() on each alone; histories and solutions are compared here bit for bit and printed as one JSON line.  A call
// with mismatched vector counts follows: it must report and leave its arguments alone.
#include <cstdio>
#include <cstring>
#include <cedar/3d/solver.h>

using namespace cedar;

static void print_hist(const char * key, const std::vector<real_t> & h)
{
	std::printf("\"%s\": [", key);
	for (std::size_t i = 0; i < h.size(); i++) std::printf("%s%.17g", i ? ", " : "", h[i]);
	std::printf("], ");
}

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	const len_t n = 33;
	const int nrhs = 3;
	auto so = cdr3::gallery::fe(n, n, n);
	std::vector<cdr3::grid_func> b, x;
	for (int m = 0; m < nrhs; m++) {
		b.emplace_back(n, n, n);
		x.emplace_back(n, n, n);
		for (len_t k = 1; k <= n; k++)
			for (len_t j = 1; j <= n; j++)
				for (len_t i = 1; i <= n; i++)
					b[m](i, j, k) = m == 0 ? 1.0 / (1.0 + i + 2.0 * j + 3.0 * k)
					              : m == 1 ? ((i * 7 + j * 13 + k * 29) % 17) - 8.0 : 1e-3 * (((i * 5 + j * 3 + k * 11) % 7) - 3.0);
	}
	cdr3::solver<cdr3::xxvii_pt> s(so, conf);
	s.pcg_many(b, x);
	std::printf("{\"iters\": [");
	for (int m = 0; m < nrhs; m++) std::printf("%s%d", m ? ", " : "", (int)s.iterations.size() > m ? s.iterations[m] : -1);
	std::printf("], ");
	const std::vector<std::vector<real_t>> many = s.histories;
	for (int m = 0; m < nrhs; m++) {
		const std::string key = "many" + std::to_string(m);
		print_hist(key.c_str(), (int)many.size() > m ? many[m] : std::vector<real_t>());
	}
	bool same_x = true;
	for (int m = 0; m < nrhs; m++) {
		cdr3::grid_func x1(n, n, n);
		s.pcg(b[m], x1);
		const std::string key = "single" + std::to_string(m);
		print_hist(key.c_str(), s.history);
		same_x = same_x && std::memcmp(x1.data(), x[m].data(), x1.size() * sizeof(real_t)) == 0;
	}
	// mismatched counts: reported, nothing computed
	std::vector<cdr3::grid_func> two;
	two.emplace_back(n, n, n);
	two.emplace_back(n, n, n);
	s.pcg_many(b, two);
	std::printf("\"same_x\": %s, \"mismatch_histories\": %d, \"mismatch_iterations\": %d}\n", same_x ? "true" : "false",
	            (int)s.histories.size(), (int)s.iterations.size());
	return 0;
}
